"""Device buffers for the GPU tests: Hip, the ctypes wrapper round the HIP runtime that the stateless-entry-point tests upload through;
zeros and put, its torch-side twins for the hand-driven paths; and the two small helpers every pipeline test file had a copy of."""
import ctypes as C

import numpy as np

_CACHE = {}


def cached(key, make):
    """make() once per process and key. One dict serves every test module: a key names its content, not the module that asked."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def copy_out(out):
    """A mapper result detached from the slot's pinned buffers."""
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


class Hip:
    """The HIP runtime the library already loaded, through ctypes: device buffers for the stateless entry points. `with Hip() as h:`
    frees them at the end."""

    def __init__(self):
        from aim_amd import capi
        capi.load()
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.lib = C.CDLL(path)
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def up(self, arr, slack=0):
        a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        a = np.concatenate([a, np.zeros(slack, dtype=np.uint8)]) if slack else a
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(len(a), 4)) == 0
        self.bufs.append(p)
        if len(a):
            assert self.lib.hipMemcpy(p, a.ctypes.data, len(a), 1) == 0
        return p

    def alloc(self, nbytes, fill=None):
        """A raw allocation of at least 256 bytes, every byte set to `fill` where one is given."""
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(int(nbytes), 256)) == 0
        self.bufs.append(p)
        if fill is not None:
            assert self.lib.hipMemset(p, fill, max(int(nbytes), 256)) == 0
        return p

    def filled(self, nbytes, byte=0xEE):
        """An uploaded buffer of nbytes, prefilled: what an output has to overwrite."""
        return self.up(np.full(nbytes, byte, dtype=np.uint8))

    def down(self, p, nbytes):
        out = np.zeros(nbytes, dtype=np.uint8)
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(out.ctypes.data, p, nbytes, 2) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.lib.hipFree(p)
        self.bufs = []


def zeros(nbytes, dev):
    """A zeroed uint8 torch tensor of at least 16 bytes (an entry point refuses a null buffer even where it needs none)."""
    import torch
    return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def put(array, dev, slack=0):
    """The array's bytes as a uint8 torch tensor on the device, `slack` zero bytes behind them."""
    import torch
    a = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    if not slack:
        return torch.from_numpy(a.copy()).to(dev)
    t = torch.zeros(len(a) + slack, dtype=torch.uint8, device=dev)
    t[:len(a)] = torch.from_numpy(a.copy()).to(dev)
    return t
