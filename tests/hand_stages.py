"""The pipeline's stages driven by hand, for the tests that compare the mapper (or a later stage) with them. Two families: the chain
kernels through the stateless entry points on Hip buffers that never leave the device in between, and the engine-dict path on torch
buffers from the candidates to the SAM records, one synchronize per stage. Test code: what the stages give is asserted where it is
used."""
import numpy as np

from gpu_buffers import Hip, put, zeros

DEV = "cuda:0"


# ---- the chain kernels on Hip buffers ----------------------------------------------------------------------------------------------
def _chain_classify(h, case, rows, rl, read_size, max_hits, mask_q8=128):
    """aim_seed_chain_device (max_hits: aim_seed_chain_long_device) and aim_chain_classify_device over seed_model's reference, every
    output prefilled with 0xEE: the device buffers by name."""
    from pipeline_batches import reference
    from aim_amd import engine
    k, stride, w, max_occ, band, flank, min_votes, K = case
    ref = reference()
    sp = engine.seed_params(k, read_size, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w,
                            long_reads=max_hits is not None)
    bucket, pos = engine.build_index(ref, k, threads=4) if w is None else engine.index_build_minimizers(ref, k, w, threads=4)
    n = len(rl)
    d = dict(rl=h.up(np.ascontiguousarray(rl, dtype=np.int32)), rows=h.up(np.ascontiguousarray(rows), 64), req=h.filled(n * K * 16), tp=h.filled(n * K * 8),
             votes=h.filled(n * K * 4), seed=h.filled(n * 16), chains=h.filled(n * K * 16), cls=h.filled(n * K * 8))
    args = (n, d["rl"], d["rows"], h.up(bucket), h.up(pos), len(ref), d["req"], d["tp"], d["votes"], d["seed"], d["chains"])
    if max_hits is None:
        engine.seed_chain_device(sp, *args)
    else:
        engine.seed_chain_long_device(sp, max_hits, *args)
    engine.chain_classify_device(K, read_size, mask_q8, n, d["rl"], d["tp"], d["seed"], d["chains"], d["cls"])
    return d


def _chain_rows(h, d, n, K):
    from aim_amd import capi
    return (h.down(d["req"], n * K * 16).view(capi.REQUEST_DTYPE), h.down(d["tp"], n * K * 8).view(np.uint64), h.down(d["seed"], n * 16).view(capi.SEED_DTYPE),
            h.down(d["chains"], n * K * 16).view(capi.CHAIN_DTYPE), h.down(d["cls"], n * K * 8).view(capi.CHAIN_CLASS_DTYPE))


def chain_then_classify(case, rows, rl, read_size, max_hits=None, mask_q8=128):
    """The chain kernel and the classification on the buffers it wrote, which never leave the device in between. Returns (requests,
    text_pos, seed rows, chains, class rows)."""
    with Hip() as h:
        return _chain_rows(h, _chain_classify(h, case, rows, rl, read_size, max_hits, mask_q8), len(rl), case[7])


def chain_classify_split(case, rows, rl, read_size, max_hits=None):
    """chain_then_classify with aim_split_segments_device behind it on the same buffers. Returns (requests, text_pos, seed, chains,
    class) and the four segment outputs."""
    from pipeline_batches import reference
    from aim_amd import capi, engine
    K, flank, n = case[7], case[5], len(rl)
    with Hip() as h:
        s_req, s_tp, s_pat, s_seg = h.filled(n * K * 16), h.filled(n * K * 8), h.filled(n * K * read_size + 64), h.filled(n * K * 8)
        d = _chain_classify(h, case, rows, rl, read_size, max_hits)
        engine.split_segments_device(K, read_size, flank, len(reference()), n, d["rl"], d["rows"], d["req"], d["tp"], d["seed"], d["chains"], d["cls"],
                                     s_req, s_tp, s_pat, s_seg)
        seg = (h.down(s_req, n * K * 16).view(capi.REQUEST_DTYPE), h.down(s_tp, n * K * 8).view(np.uint64),
               h.down(s_pat, n * K * read_size).reshape(n * K, read_size), h.down(s_seg, n * K * 8).view(capi.SEGMENT_DTYPE))
        return _chain_rows(h, d, n, K), seg


# ---- the engine-dict path on torch buffers -----------------------------------------------------------------------------------------
def wfa_params(max_score, read_size, x, o, e, free):
    """WFA (x, o, e) with BACKTRACE | ENDSFREE | REF_TEXTS and `free` bases of free text at both ends: the segment rows' alignment."""
    from aim_amd import engine
    return engine.make_params("wfa", max_score, read_size, mismatch=x, gap_o=o, gap_e=e, backtrace=True, ref_texts=True, ends_free=(0, 0, free, free))


def segment_rows(sp, ref, rl, rows, extend=None):
    """seed_chain_candidates over the host-built minimizer index of sp's (k, w), chain_classify and split_segments, then extend_segments
    where extend = (the reference on the device, aim_extend_params_t): the engine's dict."""
    from aim_amd import engine
    index = engine.index_build_minimizers(ref, sp.k, sp.options >> 8)
    out = engine.split_segments(sp, engine.chain_classify(sp, engine.seed_chain_candidates(sp, index, len(ref), rl, rows)), len(ref))
    if extend is not None:
        out = engine.extend_segments(sp, out, extend[0][:len(ref)], extend[1])
    return out


def clip_contigs(out, K, rs, flank, ref_len, starts, lens, n):
    """aim_contig_clip_device over segment_rows' dict, in place, d_contig prefilled with 0xEEEEEEEE: the device tensors (contig per slot,
    contig starts, contig lengths)."""
    import torch
    from aim_amd import engine
    d_st, d_ln = torch.from_numpy(starts.view(np.int32)).to(DEV), torch.from_numpy(lens.view(np.int32)).to(DEV)
    d_ct = torch.full((n * K,), -286331154, dtype=torch.int32, device=DEV)        # 0xEEEEEEEE
    torch.cuda.synchronize()
    engine.contig_clip_device(K, rs, flank, ref_len, len(starts), d_st.data_ptr(), d_ln.data_ptr(), n, out["d_read_len"].data_ptr(), out["d_req"].data_ptr(),
                              out["d_text_pos"].data_ptr(), out["d_chains"].data_ptr(), out["d_seg_req"].data_ptr(), out["d_seg_text_pos"].data_ptr(),
                              out["d_seg"].data_ptr(), d_ct.data_ptr())
    torch.cuda.synchronize()
    return d_ct, d_st, d_ln


def align_rows(params, count, d_req, d_pat, d_tp, d_ref, ref_len):
    """aim_align_device_ref over `count` rows: the device tensors (result rows, ops rows)."""
    import torch
    from aim_amd import capi
    lib = capi.load()
    d_res, d_ops = zeros(count * capi.RESULT_DTYPE.itemsize, DEV), zeros(count * 2 * params.read_size + 64, DEV)
    sb = lib.aim_scratch_bytes(capi.params_ref(params), count)
    d_scr = zeros(sb, DEV)
    torch.cuda.synchronize()
    rc = lib.aim_align_device_ref(capi.params_ref(params), count, d_req.data_ptr(), d_pat.data_ptr(), d_tp.data_ptr(), d_ref.data_ptr(), ref_len, d_res.data_ptr(),
                                  d_ops.data_ptr(), d_scr.data_ptr(), sb, None)
    assert rc == 0, lib.aim_last_error()
    torch.cuda.synchronize()
    return d_res, d_ops


def sam_rows(params, count, d_req, d_tp, d_res, d_ops, d_ref, ref_len, caps, split_seg=None, into=None):
    """aim_sam_device over aligned rows (split_seg, the device aim_segment_t rows: aim_sam_device_split) with capacities caps =
    (CIGAR words, MD bytes). into = (d_cigar, d_md, first word, first byte): the call writes there, behind what an earlier call has
    in the same buffers, instead of into buffers of its own. Returns the device tensors d_sam, d_cigar, d_md, d_cur and, downloaded
    after a synchronize, sam (`count` records), cigar and md (the whole buffers) and cur (the two cursors)."""
    import torch
    from aim_amd import capi, engine
    ccap, mcap = caps
    d_cigar, d_md, word0, byte0 = into if into is not None else (zeros(ccap * 4, DEV), zeros(mcap, DEV), 0, 0)
    d_sam, d_cur = zeros(count * 48, DEV), zeros(8, DEV)
    args = (params, count, d_req.data_ptr(), d_tp.data_ptr(), None, d_res.data_ptr(), d_ops.data_ptr(), d_ref.data_ptr(), ref_len, 0, d_sam.data_ptr(),
            d_cigar.data_ptr() + 4 * word0, ccap, d_md.data_ptr() + byte0, mcap, d_cur.data_ptr())
    if split_seg is None:
        engine.sam_device(*args)
    else:
        engine.sam_device_split(*args, split_seg.data_ptr())
    torch.cuda.synchronize()
    return dict(d_sam=d_sam, d_cigar=d_cigar, d_md=d_md, d_cur=d_cur, sam=d_sam.cpu().numpy().view(capi.SAM_DTYPE)[:count].copy(),
                cigar=d_cigar.cpu().numpy().view(np.uint32), md=d_md.cpu().numpy(), cur=d_cur.cpu().numpy().view(np.uint32)[:2])


def segment_records(params, out, count, d_ref, ref_len):
    """align_rows over all segment rows of segment_rows' dict and sam_rows with their segments, at capacities of 64 words and 256 bytes
    per row: (d_res, d_ops, what sam_rows returns)."""
    d_res, d_ops = align_rows(params, count, out["d_seg_req"], out["d_seg_patterns"], out["d_seg_text_pos"], d_ref, ref_len)
    return d_res, d_ops, sam_rows(params, count, out["d_seg_req"], out["d_seg_text_pos"], d_res, d_ops, d_ref, ref_len, (count * 64, count * 256), split_seg=out["d_seg"])


def single_end(extend):
    """The shared mapper batch (tests/mapper_batch.py) stage by stage, then the record model over the downloaded rows: a dict shaped like
    a mapper result."""
    import chain_class_model as ccm
    import map_records_model as mm
    import mapper_batch as mb
    from aim_amd import engine
    b = mb.batch()
    ref, rows, rl = b["ref"], b["rows"], b["read_len"]
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    rs, n = ccm.CHIMERIC_SIZE, len(rl)
    params = wfa_params(mb.max_score(), rs, mb.X, mb.O, mb.E, 2 * flank)
    d_ref = put(ref, DEV, 64)
    sp = engine.seed_params(k, rs, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    out = segment_rows(sp, ref, rl, rows, extend=(d_ref, engine.extend_params(*mb.EXTEND)) if extend else None)
    s = segment_records(params, out, n * K, d_ref, len(ref))[2]
    off, rec = mm.map_records(K, n, out["seg"], s["sam"], out["class"])
    return {"records": rec, "rec_offsets": off, "cigar": s["cigar"], "md": s["md"]}
