"""python -m aim_amd.map --ref REF.fa --reads READS.fq|.fa -o OUT.sam

Maps single-end reads against a reference with engine.Mapper (chain -> classify -> split -> [extend] -> align -> SAM
records -> record list, all on the device) and writes SAM with aim_amd.samout. Two slots are driven alternately: while one batch is
on the device the previous one is written. Bases are upper-cased on the way in (the index holds upper-case A C G T only). Without
--contigs the reference is a FASTA of ONE sequence and a FASTA with more is refused; with --contigs every sequence of the FASTA is a
contig (rule 13c of include/aim_hip.h): one @SQ line each, and every record lies inside the sequence it names."""
import argparse
import sys

import numpy as np


def read_fasta(path):
    """[(name, sequence bytes)] of a FASTA file; the name is the header up to the first white space."""
    out, name, parts = [], None, []
    with open(path, "rb") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith(b">"):
                if name is not None:
                    out.append((name, b"".join(parts)))
                head = line[1:].split()
                name, parts = (head[0].decode("latin-1") if head else ""), []
            elif name is None:
                raise ValueError("%s: sequence data before the first '>' line" % path)
            else:
                parts.append(line)
    if name is not None:
        out.append((name, b"".join(parts)))
    return out


def read_fastq(path):
    """[(name, sequence bytes, quality string)] of a four-line-per-record FASTQ file."""
    out = []
    with open(path, "rb") as f:
        lines = [l.rstrip(b"\r\n") for l in f]
    while lines and not lines[-1]:
        lines.pop()
    if len(lines) % 4:
        raise ValueError("%s: %d lines are no whole number of four-line FASTQ records" % (path, len(lines)))
    for i in range(0, len(lines), 4):
        h, s, p, q = lines[i:i + 4]
        if not h.startswith(b"@") or not p.startswith(b"+"):
            raise ValueError("%s: record %d does not start with '@' and '+' lines" % (path, i // 4))
        if len(q) != len(s):
            raise ValueError("%s: record %d has %d bases and %d qualities" % (path, i // 4, len(s), len(q)))
        head = h[1:].split()
        out.append((head[0].decode("latin-1") if head else "", s, q.decode("latin-1")))
    return out


def read_reads(path):
    """FASTQ or FASTA by the file's first byte: [(name, sequence bytes, quality string or None)]."""
    with open(path, "rb") as f:
        first = f.read(1)
    if first == b"@":
        return read_fastq(path)
    if first == b">":
        return [(n, s, None) for n, s in read_fasta(path)]
    if not first:
        return []
    raise ValueError("%s: neither FASTA ('>') nor FASTQ ('@')" % path)


def mate_name(name):
    """A read's name without a trailing /1 or /2."""
    return name[:-2] if name.endswith(("/1", "/2")) else name


def pair_reads(reads1, reads2):
    """The two files of a paired-end run as one list, mates next to each other (reads 2m and 2m + 1), under the name they share."""
    if len(reads1) != len(reads2):
        raise ValueError("--reads holds %d reads and --reads2 %d" % (len(reads1), len(reads2)))
    out = []
    for i, (a, b) in enumerate(zip(reads1, reads2)):
        if mate_name(a[0]) != mate_name(b[0]):
            raise ValueError("read %d: the mates' names differ: %r and %r" % (i, a[0], b[0]))
        out += [(mate_name(a[0]),) + tuple(a[1:]), (mate_name(b[0]),) + tuple(b[1:])]
    return out


def load_reference(path):
    """(name, upper-cased uint8 array) of a FASTA with exactly one sequence; ValueError for none or several."""
    seqs = read_fasta(path)
    if len(seqs) != 1:
        raise ValueError("%s holds %d sequences: the mapper takes a reference of one sequence (a contig table is not in this version)" % (path, len(seqs)))
    return seqs[0][0], np.frombuffer(seqs[0][1].upper(), dtype=np.uint8).copy()


def load_contigs(path):
    """(names, upper-cased uint8 arrays) of a FASTA with one sequence or more, in file order; ValueError for none or an empty one."""
    seqs = read_fasta(path)
    if not seqs:
        raise ValueError("%s holds no sequence" % path)
    for name, s in seqs:
        if not s:
            raise ValueError("%s: sequence '%s' is empty" % (path, name))
    return [n for n, _ in seqs], [np.frombuffer(s.upper(), dtype=np.uint8).copy() for _, s in seqs]


def parser():
    ap = argparse.ArgumentParser(prog="python -m aim_amd.map", description=__doc__.split("\n\n")[1])
    ap.add_argument("--ref", required=True)
    ap.add_argument("--reads", required=True)
    ap.add_argument("--reads2", default=None, help="the second mates, read by read (paired-end: rule 14c); names agree after a trailing /1 or /2")
    ap.add_argument("--min-span", type=int, default=0, help="paired-end: the smallest span of a proper pair, from the forward start to the reverse end")
    ap.add_argument("--max-span", type=int, default=1000, help="paired-end: the largest span of a proper pair")
    ap.add_argument("--unpaired-penalty", type=int, default=17, help="paired-end: what the two best single placements pay against a proper pair")
    ap.add_argument("--rescue-size", type=int, default=None, help="paired-end: row size of the rescue alignment (default: max_span - min_span + read_size, rounded up to 8)")
    ap.add_argument("--no-rescue", action="store_true", help="paired-end: pair what was mapped, rescue nothing")
    ap.add_argument("--estimate-span", action="store_true",
                    help="paired-end: estimate the span bounds from each batch on the device (rule 15c); --min-span / --max-span are the fallback and size --rescue-size")
    ap.add_argument("--est-hist-size", type=int, default=2048, help="--estimate-span: bins of one base, a multiple of 64 in 64..8192")
    ap.add_argument("--est-min-samples", type=int, default=64, help="--estimate-span: fewer sampled pairs in a batch give the fallback")
    ap.add_argument("--est-min-mapq", type=int, default=20, help="--estimate-span: the MAPQ either mate of a sample needs")
    ap.add_argument("--est-min-slack", type=int, default=16, help="--estimate-span: a floor for the spread, 3 * IQR")
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--contigs", action="store_true", help="map against every sequence of a multi-sequence FASTA (a contig table)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch", type=int, default=4096, help="reads per batch (max_reads)")
    ap.add_argument("--read-size", type=int, default=None, help="row size, a multiple of 8 (default: the longest read rounded up)")
    ap.add_argument("-k", type=int, default=12)
    ap.add_argument("-w", type=int, default=5, help="minimizer window")
    ap.add_argument("--max-occ", type=int, default=16)
    ap.add_argument("--band", type=int, default=64)
    ap.add_argument("--flank", type=int, default=8)
    ap.add_argument("--min-votes", type=int, default=2)
    ap.add_argument("--max-cands", type=int, default=4, help="K")
    ap.add_argument("--max-hits", type=int, default=None, help="0: the short-read chain kernel; else the long kernel's hit cap (default by read size)")
    ap.add_argument("--mask-q8", type=int, default=128)
    ap.add_argument("--extend", action="store_true", help="extend the inner sides of split segments to the breakpoint")
    ap.add_argument("--ext-match", type=int, default=1)
    ap.add_argument("--ext-mismatch", type=int, default=3)
    ap.add_argument("--ext-gap-o", type=int, default=4)
    ap.add_argument("--ext-gap-e", type=int, default=1)
    ap.add_argument("--xdrop", type=int, default=20)
    ap.add_argument("--ext-max-cost", type=int, default=400)
    ap.add_argument("--ext-band", type=int, default=31)
    ap.add_argument("--max-ext", type=int, default=64)
    ap.add_argument("--mismatch", type=int, default=3)
    ap.add_argument("--gap-o", type=int, default=4)
    ap.add_argument("--gap-e", type=int, default=1)
    ap.add_argument("--max-score", type=int, default=None, help="WFA cost cap of a segment (default: max(32, read_size / 10))")
    ap.add_argument("--secondary", type=int, default=0, metavar="N",
                    help="align up to N secondaries of every locus next to its primary (rule 16c, 1..15): the best copy by alignment, MAPQ from the runner-up")
    ap.add_argument("--no-secondary-lines", action="store_true", help="--secondary: do not write the copies that lost as 0x100 lines")
    ap.add_argument("--eqx", action="store_true", help="'=' and 'X' instead of 'M'")
    ap.add_argument("--cigar-cap", type=int, default=None)
    ap.add_argument("--md-cap", type=int, default=None)
    return ap


def mapper_params_from(args, read_size):
    from . import capi, engine
    long_reads = read_size > capi.SEED_MAX_READ_SIZE
    max_hits = args.max_hits if args.max_hits is not None else (4096 if long_reads else 0)
    sp = engine.seed_params(args.k, read_size, max_occ=args.max_occ, band=args.band, flank=args.flank, min_votes=args.min_votes, max_cands=args.max_cands,
                            w=args.w, long_reads=max_hits != 0)
    ep = engine.extend_params(args.ext_match, args.ext_mismatch, args.ext_gap_o, args.ext_gap_e, args.xdrop, args.ext_max_cost, args.ext_band,
                              args.max_ext) if args.extend else None
    max_score = args.max_score if args.max_score is not None else max(32, read_size // 10)
    return engine.mapper_params(sp, args.batch, max_score, mismatch=args.mismatch, gap_o=args.gap_o, gap_e=args.gap_e, max_hits=max_hits, mask_q8=args.mask_q8,
                                extend=ep, sam_options=capi.SAM_EQX if args.eqx else 0, slots=2, cigar_cap=args.cigar_cap, md_cap=args.md_cap)


def main(argv=None):
    args = parser().parse_args(argv)
    try:
        if args.contigs:
            rname, ref = load_contigs(args.ref)
            ref_lens = [len(s) for s in ref]
        else:
            rname, ref = load_reference(args.ref)
            ref_lens = len(ref)
        reads = read_reads(args.reads)
        if args.reads2:
            reads = pair_reads(reads, read_reads(args.reads2))
            if args.batch % 2:
                raise ValueError("--batch %d must be even with --reads2 (mates share a batch)" % args.batch)
    except (OSError, ValueError) as e:
        hint = "; --contigs maps against all of them" if not args.contigs and "contig table" in str(e) else ""
        print("aim_amd.map: %s%s" % (e, hint), file=sys.stderr)
        return 2
    from . import capi, engine, samout
    longest = max([len(s) for _, s, _ in reads] + [1])
    read_size = args.read_size if args.read_size is not None else engine.round_up_8(longest)
    if longest > read_size:
        print("aim_amd.map: a read of %d bases does not fit --read-size %d" % (longest, read_size), file=sys.stderr)
        return 2
    try:
        mp = mapper_params_from(args, read_size)
    except ValueError as e:
        print("aim_amd.map: %s" % e, file=sys.stderr)
        return 2
    n_lines = 0
    make = engine.Mapper.from_contigs if args.contigs else engine.Mapper
    with open(args.out, "w") as fh, make(mp, ref, device=args.device) as m:
        if args.reads2:
            span = args.max_span - args.min_span + read_size
            pp = engine.pair_params(args.min_span, args.max_span, args.unpaired_penalty, rescue=not args.no_rescue,
                                    rescue_size=args.rescue_size if args.rescue_size is not None else engine.round_up_8(max(span, read_size)),
                                    rescue_cigar_cap=args.batch * 64, rescue_md_cap=args.batch * 256)
            est = engine.pair_estimate_params(args.est_hist_size, args.est_min_samples, args.est_min_mapq, args.est_min_slack) if args.estimate_span else None
            try:
                if args.secondary:                    # rule 17c: pairing over the aligned secondaries, MAPQ from the pair's runner-up
                    m.set_pairing_secondary(pp, engine.secondary_params(args.secondary, records=not args.no_secondary_lines), estimate=est)
                else:
                    m.set_pairing(pp, estimate=est)
            except capi.AimError as e:
                print("aim_amd.map: %s" % e, file=sys.stderr)
                return 2
        elif args.secondary:
            try:
                m.set_secondary(engine.secondary_params(args.secondary, records=not args.no_secondary_lines))
            except capi.AimError as e:
                print("aim_amd.map: %s" % e, file=sys.stderr)
                return 2
        fh.write(samout.header(rname, ref_lens, command_line=" ".join(["python -m aim_amd.map"] + list(sys.argv[1:] if argv is None else argv))))
        pending = {}                                  # slot -> the batch in flight on it

        def finish(slot):
            nonlocal n_lines
            names, rows, rl, quals = pending.pop(slot)
            out = m.wait(slot)
            if out["cigar_needed"] > mp.cigar_cap or out["md_needed"] > mp.md_cap:
                print("aim_amd.map: a batch needed %d CIGAR words and %d MD bytes: records over --cigar-cap %d / --md-cap %d have no CIGAR" %
                      (out["cigar_needed"], out["md_needed"], mp.cigar_cap, mp.md_cap), file=sys.stderr)
            if "pair_estimate" in out:
                e = out["pair_estimate"]
                print("aim_amd.map: span estimate p25=%d p50=%d p75=%d bounds=%d..%d samples=%d beyond=%d flags=0x%x" %
                      (e["p25"], e["p50"], e["p75"], e["min_span"], e["max_span"], e["n_samples"], e["n_beyond"], e["flags"]), file=sys.stderr)
            n_lines += samout.write(fh, out, names, rows, rl, rname, quals)
        for b, lo in enumerate(range(0, len(reads), args.batch)):
            part = reads[lo:lo + args.batch]
            slot = b & 1                              # (free: its previous batch was written while the last one ran)
            rows = np.zeros((len(part), read_size), dtype=np.uint8)
            rl = np.zeros(len(part), dtype=np.int32)
            for i, (_, s, _) in enumerate(part):
                rows[i, :len(s)] = np.frombuffer(s.upper(), dtype=np.uint8)
                rl[i] = len(s)
            m.submit(slot, rl, rows)
            pending[slot] = ([n for n, _, _ in part], rows, rl, [q for _, _, q in part])
            if (slot ^ 1) in pending:                 # the older batch: written while this one runs
                finish(slot ^ 1)
        for slot in list(pending):                    # the last batch
            finish(slot)
    print("aim_amd.map: %d reads, %d SAM lines -> %s" % (len(reads), n_lines, args.out), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
