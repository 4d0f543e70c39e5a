"""The rule of AIM_FLAG_SAM_FIELDS (include/aim_hip.h) in plain Python: one ops range of one row -> the SAM fields.

AIM 'I' consumes a text (= reference) base and is SAM 'D'; AIM 'D' consumes a pattern (= read) base and is SAM 'I'. A strand-1 row is
taken in reverse order; reference bases are read from the forward reference at their forward position."""
import numpy as np

BAM_M, BAM_I, BAM_D, BAM_S, BAM_EQ, BAM_X = 0, 1, 2, 4, 7, 8
BAM_CHARS = "MIDNSHP=X"
SAM_EQX, SAM_REVERSE, SAM_UNMAPPED, SAM_OVERFLOW = 0x1, 0x10, 0x4, 0x100
UNMAPPED = None


def sam_fields(ops, begin, end, strand, window_start, reference, eqx=False):
    """(pos, ref_span, nm, cigar words, md bytes, flags) of ops[begin:end]; an unmapped row (empty range, or nothing left after the
    terminal runs are peeled) gives (window_start, 0, 0, [], b"", SAM_UNMAPPED)."""
    walk = bytes(bytearray(ops[begin:end]))
    if strand:
        walk = walk[::-1]
    k0, k1 = 0, len(walk)
    while k0 < k1 and walk[k0:k0 + 1] not in (b"M", b"X"):
        k0 += 1
    while k1 > k0 and walk[k1 - 1:k1] not in (b"M", b"X"):
        k1 -= 1
    if k1 <= k0:
        return int(window_start), 0, 0, [], b"", SAM_UNMAPPED
    lead, core, trail = walk[:k0], walk[k0:k1], walk[k1:]
    pos = int(window_start) + lead.count(b"I")
    runs = []   # [bam op, length]

    def push(op, n=1):
        if n:
            if runs and runs[-1][0] == op:
                runs[-1][1] += n
            else:
                runs.append([op, n])

    push(BAM_S, len(lead) - lead.count(b"I"))
    md = bytearray()
    count, rp, nm, in_del = 0, pos, 0, False
    for c in core:
        c = chr(c)
        if c == "M":
            push(BAM_EQ if eqx else BAM_M)
            count += 1
            rp += 1
        elif c == "X":
            push(BAM_X if eqx else BAM_M)
            md += b"%d" % count + bytes([reference[rp]])
            count, rp, nm = 0, rp + 1, nm + 1
        elif c == "I":
            push(BAM_D)
            if not in_del:
                md += b"%d^" % count
                count = 0
            md.append(reference[rp])
            rp, nm = rp + 1, nm + 1
        else:
            push(BAM_I)
            nm += 1
        in_del = c == "I"
    md += b"%d" % count
    # (the clip is pushed after the core: it never merges with it, S being no core op)
    push(BAM_S, len(trail) - trail.count(b"I"))
    words = [(n << 4) | op for op, n in runs]
    return pos, rp - pos, nm, words, bytes(md), (SAM_REVERSE if strand else 0)


def row_fields(res_row, ops_row, text_pos, reference, algo_is_wfa, max_score, eqx=False, read_size=None):
    """sam_fields of one result row, or the unmapped record: status not OK, an empty range, a WFA row over the cap, or no candidate
    (text_pos None)."""
    if text_pos is None:
        return 0, 0, 0, [], b"", SAM_UNMAPPED
    ws, strand = int(text_pos) & ((1 << 63) - 1), int(text_pos) >> 63
    b, e = int(res_row["begin_offset"]), int(res_row["end_offset"])
    if int(res_row["status"]) != 0 or e <= b or (algo_is_wfa and int(res_row["score"]) == max_score + 1):
        return ws, 0, 0, [], b"", SAM_UNMAPPED
    return sam_fields(ops_row, b, e, strand, ws, reference, eqx)


def cigar_string(words):
    return "".join("%d%s" % (w >> 4, BAM_CHARS[w & 15]) for w in words) or "*"


def check_records(sam, cigar, md, expect, skip_overflow=False):
    """Compare records (capi.SAM_DTYPE) and the content their offsets address with a list of sam_fields tuples; returns the rows marked
    SAM_OVERFLOW (compared on every field but the content)."""
    over = []
    cigar, md = np.asarray(cigar), np.asarray(md, dtype=np.uint8)
    for i, (pos, span, nm, words, mdb, flags) in enumerate(expect):
        r = sam[i]
        assert (int(r["pos"]), int(r["ref_span"]), int(r["nm"]), int(r["flags"]), int(r["pad"])) == (pos, span, nm, flags, 0), (i, r, expect[i])
        if int(r["status"]) & SAM_OVERFLOW:
            assert skip_overflow, (i, r)
            assert int(r["n_cigar"]) == 0 and int(r["md_len"]) == 0 and words, (i, r)
            over.append(i)
            continue
        co, nc, mo, ml = int(r["cigar_offset"]), int(r["n_cigar"]), int(r["md_offset"]), int(r["md_len"])
        assert [int(w) for w in cigar[co:co + nc]] == words, (i, cigar_string(cigar[co:co + nc]), cigar_string(words))
        assert md[mo:mo + ml].tobytes() == mdb, (i, md[mo:mo + ml].tobytes(), mdb)
    return over


def rebuild_reference(read, words, md, strict=False):
    """The reference slice [pos, pos + ref_span) from the READ, the CIGAR and the MD (what samtools does the other way round): the
    round trip that checks the model against something other than itself. `read` is in forward-strand orientation. strict: a
    mismatch's reference byte must differ from the read's (WFA; the NW / SWG traceback, like the reference's, may print 'X' over two
    equal bases when a mismatch and another path tie, and the record repeats what the ops say)."""
    import re
    toks = re.findall(rb"\d+|\^[^0-9]+|[^0-9^]", md)
    out = bytearray()
    rd = 0
    # MD as a stream over the reference-consuming ops: ('=', n) | ('X', byte) | ('D', bytes)
    stream = []
    for t in toks:
        if t[:1].isdigit():
            stream.append(["=", int(t)])
        elif t[:1] == b"^":
            stream.append(["D", bytearray(t[1:])])
        else:
            stream.append(["X", t[0]])
    si = 0
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        if op in (BAM_S, BAM_I):
            rd += n
        elif op == BAM_D:
            while si < len(stream) and stream[si][0] == "=" and stream[si][1] == 0:
                si += 1
            assert stream[si][0] == "D" and len(stream[si][1]) == n, (stream[si], n)
            out += stream[si][1]
            si += 1
        else:
            left = n
            while left:
                while stream[si][0] == "=" and stream[si][1] == 0:
                    si += 1
                kind = stream[si][0]
                if kind == "=":
                    take = min(left, stream[si][1])
                    assert op != BAM_X
                    out += read[rd:rd + take]
                    stream[si][1] -= take
                    rd, left = rd + take, left - take
                else:
                    assert kind == "X" and op != BAM_EQ, (stream[si], op)
                    assert not strict or read[rd] != stream[si][1]
                    out.append(stream[si][1])
                    si += 1
                    rd, left = rd + 1, left - 1
    assert all(s[0] == "=" and s[1] == 0 for s in stream[si:]), stream[si:]
    return bytes(out), rd


# ---- what the record tests share ------------------------------------------------------------------------------------------------
def make_reference(seed, n=300000):
    """Random A/C/G/T with a few N runs and lowercase stretches (the MD carries reference bytes verbatim)."""
    rng = np.random.default_rng([seed, 0x73616D])
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    for _ in range(n // 20000):
        at = int(rng.integers(0, n - 600))
        ref[at:at + int(rng.integers(1, 12))] = ord("N")
        at = int(rng.integers(0, n - 600))
        ref[at:at + int(rng.integers(16, 300))] |= 0x20
    return ref


# hand-made ops rows: all-gap rows, alternating terminal runs, soft clips at both ends, a row longer than a wavefront's share
HAND_ROWS = [b"IIIDDDII", b"DDDD", b"IDIDDMXMDIID", b"DDIMMXMII", b"MXXMIM", b"MMIIXM", b"DDDDMMMMMMMMXMMMMMDDD", b"M" * 300 + b"I" * 70 + b"XX" + b"D" * 9 + b"M" * 1100 + b"DD"]
