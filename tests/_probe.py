"""TEST INFRASTRUCTURE: builds and binds the two halves of the lane conformance suite -- tests/probe/probe.hip for gfx950 (with the
flags of the product library, particlemdi.jl_amd/_lib.py) and tests/emu/emu_lanes.cpp for the host (built like tests/_emu.py builds
the emulator) -- into a directory the caller names (a session temporary one), and loads them with ctypes.  Both export the same
entry points for group A (the wave primitives); the device library has groups B and C as well.  A failed build raises.

A `Probe` calls an entry point as fn(inputs..., outputs..., sizes..., stream): numpy arrays in, numpy arrays out.  On the device
the inputs go up as torch tensors, the launcher gets data_ptr()s and the current stream, and there is one synchronize per call.
Outputs start as bytes of 0x5A, so that a value the probe never wrote is not mistaken for a zero."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "particlemdi.jl_amd", "csrc")
_INC = os.path.join(_ROOT, "include")
PROBE_HIP = os.path.join(_HERE, "probe", "probe.hip")
EMU_CPP = os.path.join(_HERE, "emu", "emu_lanes.cpp")
FILL = 0x5A


def build_device(outdir, source=PROBE_HIP, extra=()):
    """hipcc cross-compiles for gfx950 without a GPU: the flags of _lib._build_locked, in one step"""
    out = os.path.join(str(outdir), "liblane_probe.so")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-I", _CSRC, "-I", _INC,
                           "-I", os.path.dirname(PROBE_HIP)] + list(extra) + ["-shared", "-x", "hip", source, "-o", out])
    return out


def build_emu(outdir, source=EMU_CPP, extra=()):
    out = os.path.join(str(outdir), "liblane_emu.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + list(extra) + [source, "-o", out])
    return out


class Probe:
    def __init__(self, path, device):
        self.device = bool(device)
        if self.device:
            import torch      # first: the probe library must bind to the HIP runtime torch brings, to share pointers and streams
            self._torch = torch
        self._L = C.CDLL(path)

    def call(self, name, ins, outs, sizes):
        """ins: numpy arrays; outs: (shape, dtype) pairs; sizes: ints.  Returns the outputs as numpy arrays."""
        fn = getattr(self._L, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * (len(ins) + len(outs)) + [C.c_int] * len(sizes) + [C.c_void_p]
        ins = [np.ascontiguousarray(a) for a in ins]
        nbytes = [int(np.prod(shape)) * np.dtype(dt).itemsize for shape, dt in outs]
        if not self.device:
            bufs = [np.full(max(n, 1), FILL, dtype=np.uint8) for n in nbytes]
            rc = fn(*[a.ctypes.data for a in ins], *[b.ctypes.data for b in bufs], *[int(s) for s in sizes], None)
            assert rc == 0, (name, rc)
            raw = bufs
        else:
            torch = self._torch
            dev = torch.device("cuda", 0)
            up = [torch.from_numpy(a.reshape(-1).view(np.uint8).copy() if a.size else np.zeros(1, dtype=np.uint8)).to(dev) for a in ins]
            down = [torch.full((max(n, 1),), FILL, dtype=torch.uint8, device=dev) for n in nbytes]
            st = torch.cuda.current_stream(dev).cuda_stream
            rc = fn(*[t.data_ptr() for t in up], *[t.data_ptr() for t in down], *[int(s) for s in sizes], C.c_void_p(st))
            torch.cuda.synchronize()
            assert rc == 0, (name, rc)
            raw = [t.cpu().numpy() for t in down]
        return [r[:n].view(dt).reshape(shape) for r, n, (shape, dt) in zip(raw, nbytes, outs)]

    # ---- group A: the wave primitives (both libraries) ---------------------------------------------------------------------------
    def wave_reduce(self, v):
        """v [nvec][64] doubles -> sum, max, min, prev, each [nvec][64]"""
        v = np.ascontiguousarray(v, dtype=np.float64)
        return self.call("lp_wave_reduce", [v], [(v.shape, np.float64)] * 4, [len(v)])

    def wave_scan(self, v):
        v = np.ascontiguousarray(v, dtype=np.int32)
        return self.call("lp_wave_scan", [v], [(v.shape, np.int32)] * 2, [len(v)])

    def wave_shfl(self, vd, vi, src):
        vd = np.ascontiguousarray(vd, dtype=np.float64)
        return self.call("lp_wave_shfl", [vd, np.ascontiguousarray(vi, dtype=np.int32), np.ascontiguousarray(src, dtype=np.int32)],
                         [(vd.shape, np.float64), (vd.shape, np.int32)], [len(vd)])

    def wave_readlane(self, vi, vu, src):
        vi = np.ascontiguousarray(vi, dtype=np.int32)
        return self.call("lp_wave_readlane", [vi, np.ascontiguousarray(vu, dtype=np.uint64), np.ascontiguousarray(src, dtype=np.int32)],
                         [(vi.shape, np.int32), (vi.shape, np.uint64)], [len(vi)])

    def popc64(self, words, p):
        p = np.ascontiguousarray(p, dtype=np.int32)
        return self.call("lp_popc64", [np.ascontiguousarray(words, dtype=np.uint64), p], [(p.shape, np.int32)], [len(p)])[0]

    def regarr(self, idx, x, nn):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        return self.call("lp_regarr", [idx, np.ascontiguousarray(x, dtype=np.int32)], [(idx.shape + (nn,), np.int32)] * 2, [len(idx), nn])

    # ---- group B: the block primitives of pmdi_device.h (device library only) -------------------------------------------------------
    def block_excl_scan(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        return self.call("lp_block_excl_scan", [a, np.ascontiguousarray(b, dtype=np.uint64)], [(a.shape, np.uint64)] * 4, [a.shape[0], a.shape[1]])

    def block_flag_scan(self, flags):
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        return self.call("lp_block_flag_scan", [f], [(f.shape, np.uint64)] * 2, [f.shape[0], f.shape[1]])

    def block_max_sum2(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return self.call("lp_block_max_sum2", [a, np.ascontiguousarray(b, dtype=np.float64)], [(a.shape, np.float64)] * 3, [a.shape[0], a.shape[1]])

    def wave_group(self, key, valid, mode, rounds=0):
        key = np.ascontiguousarray(key, dtype=np.int32)
        return self.call("lp_wave_group", [key, np.ascontiguousarray(valid, dtype=np.uint8)], [(key.shape, np.int32)] * 2, [len(key), mode, rounds])

    def popc_below(self, words, p):
        p = np.ascontiguousarray(p, dtype=np.int32)
        return self.call("lp_popc_below", [np.ascontiguousarray(words, dtype=np.uint64), p], [(p.shape, np.int32)], [len(p)])[0]

    def jl_cumsum(self, arrays):
        """every array in place by thread 0 of its own workgroup; returns the list of results"""
        off = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int32)
        flat = np.ascontiguousarray(np.concatenate(arrays), dtype=np.float64)
        if not self.device:
            raise RuntimeError("jl_cumsum_inplace has a device probe only")
        torch = self._torch
        dev = torch.device("cuda", 0)
        c, o = torch.from_numpy(flat.copy()).to(dev), torch.from_numpy(off).to(dev)
        fn = self._L.lp_jl_cumsum
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        rc = fn(o.data_ptr(), c.data_ptr(), len(arrays), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0, rc
        out = c.cpu().numpy()
        return [out[off[i]:off[i + 1]] for i in range(len(arrays))]

    # ---- group C: the device forms of pmdi_arith.h -------------------------------------------------------------------------------
    def uniform(self, seed, words):
        """seed [nt] uint64, words [nt][5] uint32 (iter, pos, k, p, site) -> uniform01<true>, uniform01<false>"""
        seed = np.ascontiguousarray(seed, dtype=np.uint64)
        return self.call("lp_uniform", [seed, np.ascontiguousarray(words, dtype=np.uint32)], [(seed.shape, np.float64)] * 2, [len(seed)])

    def resample_u(self, u01, P):
        u01 = np.ascontiguousarray(u01, dtype=np.float64)
        return self.call("lp_resample_u", [u01], [((len(u01), P), np.float64)], [len(u01), P])[0]
