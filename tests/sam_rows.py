"""aim_sam_device and aim_sam_device_split over rows uploaded to the device, for the GPU tests of the record kernels
(test_sam_fields_gpu.py, test_split_gpu.py, test_directed_ops_gpu.py): a guard word and a guard byte sit behind each capacity."""
import numpy as np

from gpu_buffers import Hip


def sam_device(params, res, ops, tpos, ref, sel=None, options=0, ccap=1, mcap=1, req=None, ref_slack=16):
    """aim_sam_device over rows uploaded to the device: (records, words, bytes, cursors). A guard word / byte sits behind each
    capacity. ref_slack: zero bytes uploaded behind the reference (0: exactly ref_len bytes)."""
    from aim_amd import capi, engine
    with Hip() as h:
        n = len(res)
        d_res, d_ops, d_tp = h.up(res), h.up(ops, 64), h.up(np.asarray(tpos, dtype=np.uint64))
        d_ref = h.up(ref, ref_slack)
        d_req = h.up(req if req is not None else np.zeros(max(len(tpos), 1), dtype=capi.REQUEST_DTYPE))
        d_sel = None if sel is None else h.up(np.asarray(sel, dtype=np.uint32))
        d_sam = h.up(np.zeros(n * 48, dtype=np.uint8))
        d_cg = h.up(np.full(ccap + 1, 0x7E7E7E7E, dtype=np.uint32))
        d_md = h.up(np.full(mcap + 1, 0x7E, dtype=np.uint8))
        d_cur = h.up(np.full(2, 0xFFFFFFFF, dtype=np.uint32))
        engine.sam_device(params, n, d_req, d_tp, d_sel, d_res, d_ops, d_ref, len(ref), options, d_sam, d_cg, ccap, d_md, mcap, d_cur, None)
        cg, md = h.down(d_cg, 4 * (ccap + 1)).view(np.uint32), h.down(d_md, mcap + 1)
        assert int(cg[ccap]) == 0x7E7E7E7E and int(md[mcap]) == 0x7E, "written past a capacity"
        return h.down(d_sam, n * 48).view(capi.SAM_DTYPE), cg[:ccap], md[:mcap], h.down(d_cur, 8).view(np.uint32)


def sam_both(params, res, ops, tpos, ref, seg, sel=None, options=0, ccap=1, mcap=1, split_ccap=None, ref_slack=16):
    """aim_sam_device and aim_sam_device_split over the same uploaded rows: two tuples (records, words, bytes, cursors). A guard word /
    byte sits behind each capacity. split_ccap: another CIGAR capacity for the split call."""
    from aim_amd import capi, engine
    with Hip() as h:
        n = len(res)
        d_res, d_ops, d_tp, d_ref = h.up(res), h.up(ops, 64), h.up(np.asarray(tpos, dtype=np.uint64)), h.up(ref, ref_slack)
        d_req = h.up(np.zeros(max(len(tpos), 1), dtype=capi.REQUEST_DTYPE))
        d_sel = None if sel is None else h.up(np.asarray(sel, dtype=np.uint32))
        d_seg = h.up(seg)
        out = []
        for split in (False, True):
            cc = split_ccap if split and split_ccap is not None else ccap
            d_sam, d_cg, d_md = h.up(np.zeros(n * 48, dtype=np.uint8)), h.up(np.full(cc + 1, 0x7E7E7E7E, dtype=np.uint32)), h.up(np.full(mcap + 1, 0x7E, dtype=np.uint8))
            d_cur = h.up(np.full(2, 0xFFFFFFFF, dtype=np.uint32))
            args = (params, n, d_req, d_tp, d_sel, d_res, d_ops, d_ref, len(ref), options, d_sam, d_cg, cc, d_md, mcap, d_cur)
            if split:
                engine.sam_device_split(*args, d_seg, None)
            else:
                engine.sam_device(*args, None)
            cg, md = h.down(d_cg, 4 * (cc + 1)).view(np.uint32), h.down(d_md, mcap + 1)
            assert int(cg[cc]) == 0x7E7E7E7E and int(md[mcap]) == 0x7E, "written past a capacity"
            out.append((h.down(d_sam, n * 48).view(capi.SAM_DTYPE), cg[:cc], md[:mcap], h.down(d_cur, 8).view(np.uint32)))
        return out
