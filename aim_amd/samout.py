"""SAM text from the mapper's records (engine.Mapper.wait, rule 12c of include/aim_hip.h). Pure Python over numpy views; the one call
into the library is the CIGAR formatter aim_sam_format_cigar.

One line per record, in record order. Every line of a read carries the read's full SEQ (reverse-complemented on strand 1) with soft
clips, as `minimap2 -Y` writes supplementary lines: there are no hard clips. Tags: NM:i, MD:Z, AS:i and, on reads with more than one
record, SA:Z. AS is the negated alignment cost (the library's scores are penalties: 0 is a perfect match), so a greater AS is a better
alignment. MAPQ is the record's own: the chain MAPQ of rule 8c, this project's figure.

A result of a mapper with pairing (rule 14c: `out` carries "mates", one aim_map_mate_t per record) gives paired lines: FLAG is the
record's own, which already holds 0x1 / 0x2 / 0x8 / 0x20 / 0x40 / 0x80; RNEXT is `=` on the record's own contig, PNEXT 1-based and TLEN
signed, all from the mate fields; an unmapped read whose mate is mapped is written at its mate's RNAME and POS, as the SAM
specification recommends; with both reads unmapped RNAME / RNEXT are `*` and the positions 0. SA is written as before.

A result of a mapper with secondaries (rule 16c: `out` carries "sec", one aim_map_sec_t per record) marks every mapped line: `tp:A:P`
on a locus record, `tp:A:S` on a secondary record (FLAG 0x100). A secondary line has SEQ and QUAL `*`, as the SAM specification allows
for secondary alignments, MAPQ 0 and no SA tag, and the SA tags of the other lines list non-secondary records only. MAPQ of a locus
record is rule 16c's: from the alignment scores of the locus' copies, capped by the chain's anchors.

A result of a mapper with both (rule 17c, Mapper.set_pairing_secondary) carries "mates" and "sec": paired lines with `tp:A:P` /
`tp:A:S`. A `0x100` line gets the mate fields of any line -- 0x1, 0x40 / 0x80, 0x8 / 0x20, RNEXT and PNEXT -- never 0x2, TLEN 0, and
`*` for SEQ and QUAL. MAPQ of the two chosen records of a proper pair is rule 17c's, from the pair's runner-up."""
import numpy as np

from . import capi, engine

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(seq):
    """Reverse complement of bytes: A<->T, C<->G in either case, every other byte kept."""
    return bytes(seq).translate(_COMP)[::-1]


def header(rname, ref_len, command_line=None, version="1"):
    """@HD / @SQ / @PG. rname and ref_len are one sequence's name and length, or two lists, one entry per contig (rule 13c): one @SQ
    line each, in contig order."""
    pg = "@PG\tID:aim_amd\tPN:aim_amd\tVN:%s" % version
    if command_line:
        pg += "\tCL:" + command_line
    sq = [(rname, ref_len)] if isinstance(rname, str) else list(zip(rname, ref_len))
    return "@HD\tVN:1.6\tSO:unsorted\n%s%s\n" % ("".join("@SQ\tSN:%s\tLN:%d\n" % (n, int(l)) for n, l in sq), pg)


def _cigar(rec, cigar):
    s = rec["sam"]
    if int(s["status"]) & capi.SAM_OVERFLOW or not int(s["n_cigar"]):
        return "*"
    o = int(s["cigar_offset"])
    return engine.sam_format_cigar(cigar[o:o + int(s["n_cigar"])])


def _rname(rname, rec):
    """A record's RNAME: the one name, or the name of the contig in the record's pad (Mapper.from_contigs)."""
    return rname if isinstance(rname, str) else rname[int(rec["sam"]["pad"])]


def _sa(rname, rec, cigar):
    s = rec["sam"]
    return "%s,%d,%s,%s,%d,%d;" % (_rname(rname, rec), int(s["pos"]) + 1, "-" if int(s["flags"]) & capi.SAM_REVERSE else "+", _cigar(rec, cigar), int(rec["mapq"]), int(s["nm"]))


def record_lines(out, names, reads, read_len, rname, quals=None):
    """The SAM lines (without newlines) of one mapper result `out` (the dict of Mapper.wait, or anything with "records", "rec_offsets",
    "cigar" and "md"). names[r] is read r's QNAME, reads[r] its row of bases (bytes or a uint8 row), read_len[r] its length and
    quals[r] (optional) its quality string. rname is the reference's name, or the list of contig names for the records of
    Mapper.from_contigs, whose pad says which contig pos is local to; an SA entry carries its own record's contig."""
    recs, off, cigar, md = out["records"], out["rec_offsets"], out["cigar"], np.asarray(out["md"], dtype=np.uint8)
    mates = out.get("mates") if isinstance(out, dict) else None
    with_sec = isinstance(out, dict) and out.get("sec") is not None
    contig_name = lambda c: rname if isinstance(rname, str) else rname[int(c)]
    lines = []
    for r in range(len(off) - 1):
        group = recs[int(off[r]):int(off[r + 1])]
        L = int(read_len[r])
        seq = bytes(reads[r][:L]) if isinstance(reads[r], (bytes, bytearray)) else np.asarray(reads[r], dtype=np.uint8)[:L].tobytes()
        qual = quals[r] if quals is not None and quals[r] is not None else None
        # in an SA tag the non-supplementary line comes first, then the others in rank order
        sa_order = sorted((j for j in range(len(group)) if not int(group[j]["sam"]["flags"]) & capi.SAM_SECONDARY), key=lambda j: (bool(int(group[j]["sam"]["flags"]) & capi.SAM_SUPPLEMENTARY), int(group[j]["rank"])))
        for j, rec in enumerate(group):
            s = rec["sam"]
            flags = int(s["flags"])
            rnext, pnext, tlen = "*", "0", "0"
            if mates is not None:                     # rule 14c's mate fields; with an unmapped mate they are the record's own place
                mt = mates[int(off[r]) + j]
                if not (flags & capi.SAM_UNMAPPED and flags & 0x8):
                    rnext, pnext, tlen = "=", str(int(mt["mate_pos"]) + 1), str(int(mt["tlen"]))
                    if not flags & (capi.SAM_UNMAPPED | 0x8) and not isinstance(rname, str) and int(mt["mate_contig"]) != int(s["pad"]):
                        rnext = contig_name(mt["mate_contig"])
            if flags & capi.SAM_UNMAPPED:
                place = ["*", "0"] if mates is None or flags & 0x8 else [contig_name(mt["mate_contig"]), pnext]
                lines.append("\t".join([names[r], str(flags) if mates is not None else "4"] + place + ["0", "*", rnext, pnext, "0", seq.decode("latin-1") or "*", qual or "*"]))
                continue
            rev = bool(flags & capi.SAM_REVERSE)
            secondary = bool(flags & capi.SAM_SECONDARY)   # rule 16c: another copy of a locus -- no bases, no qualities, no SA
            fields = [names[r], str(flags), _rname(rname, rec), str(int(s["pos"]) + 1), str(int(rec["mapq"])), _cigar(rec, cigar), rnext, pnext, tlen,
                      "*" if secondary else (revcomp(seq) if rev else seq).decode("latin-1") or "*",
                      "*" if secondary or not qual else (qual[::-1] if rev else qual), "NM:i:%d" % int(s["nm"])]
            if int(s["md_len"]) and not int(s["status"]) & capi.SAM_OVERFLOW:
                o = int(s["md_offset"])
                fields.append("MD:Z:" + md[o:o + int(s["md_len"])].tobytes().decode("latin-1"))
            fields.append("AS:i:%d" % -int(s["score"]))
            if with_sec or secondary:
                fields.append("tp:A:S" if secondary else "tp:A:P")
            if len(sa_order) > 1 and not secondary:
                fields.append("SA:Z:" + "".join(_sa(rname, group[k], cigar) for k in sa_order if k != j))
            lines.append("\t".join(fields))
    return lines


def write(fh, out, names, reads, read_len, rname, quals=None):
    """record_lines, written to the text file `fh`; returns the number of lines."""
    lines = record_lines(out, names, reads, read_len, rname, quals)
    for line in lines:
        fh.write(line + "\n")
    return len(lines)
