"""Digests of converted bootstrapping keys, to compare two builds of the library on one machine
(DESIGN.md §4.20).

For a seeded uniform-random standard key with n = 2, each shape is converted, the device key copied back,
and one line printed: the entry point, the source (host or device, src_is_device = 1), the shape, the
SHA-256 of the key bytes and concrete_hip_key_spectrum_max as a hex float.  Shapes: the DD_SHAPES of
tests/test_gpu_key_accuracy.py through concrete_hip_convert_bsk, the first six GENERIC_SHAPES through
concrete_hip_convert_bsk_generic.  CONCRETE_HIP_LIB selects the build; two builds agree when their
outputs are equal line for line.  The host tables come from cosl, so digests of different machines
need not agree and none is kept as a fixture.

  python tools/key_digest.py                         the digest lines
  python tools/key_digest.py --time LIB_A LIB_B      concrete_hip_convert_bsk of the cfg2 key from a host
                                                     source, 5 runs per library, alternating, each
                                                     bracketed by a device synchronisation
"""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_LWE = 2


def random_key(n, k, N, l, seed):
    rng = np.random.RandomState(seed)
    w = rng.randint(0, 2 ** 32, size=(n * l * (k + 1) ** 2 * N, 2), dtype=np.int64).astype(np.uint64)
    return np.ascontiguousarray((w[:, 0] << np.uint64(32)) | w[:, 1])


def digests():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from concrete_amd import _native
    from concrete_amd import backend as B
    from test_gpu_key_accuracy import DD_SHAPES, GENERIC_SHAPES
    L = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    for general, shapes in ((False, DD_SHAPES), (True, GENERIC_SHAPES[:6])):
        name = "convert_bsk_generic" if general else "convert_bsk"
        fn = getattr(L, "concrete_hip_" + name)
        for k, N, l in shapes:
            p = B.PbsParams(n=N_LWE, k=k, N=N, level=l, base_log=1, ks_level=1, ks_base_log=1)
            nbytes = L.concrete_hip_generic_bsk_size_bytes(N_LWE, k, l, N) if general else B.fourier_bsk_bytes(p)
            assert nbytes > 0
            key = random_key(N_LWE, k, N, l, 1600 + 7 * (N % 1009) + 31 * k + l)
            d_key = B.to_device(key, "cuda:0")
            for source in ("host", "device"):
                out = torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda:0")
                src = key.ctypes.data if source == "host" else d_key.data_ptr()
                rc = fn(s, 0, out.data_ptr(), src, int(source == "device"), N_LWE, k, l, N)
                torch.cuda.synchronize()
                assert rc in (0, -2), (name, source, k, N, l, rc, L.concrete_hip_last_error())
                sha = hashlib.sha256(B.to_host(out).tobytes()).hexdigest()
                smax = float(L.concrete_hip_key_spectrum_max(out.data_ptr()))
                print(f"{name} {source} k={k} N={N} l={l} rc={rc} sha256={sha} max|G|={smax.hex()}", flush=True)


def timing(paths, reps=5):
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from concrete_amd import backend as B
    p = B.CFG2
    key = random_key(p.n, p.k, p.N, p.level, 1616)
    libs = []
    for path in paths:
        L = C.CDLL(os.path.abspath(path))
        L.concrete_hip_fourier_bsk_size_bytes.restype = C.c_uint64
        L.concrete_hip_fourier_bsk_size_bytes.argtypes = [C.c_uint32] * 4
        L.concrete_hip_convert_bsk.restype = C.c_int
        L.concrete_hip_convert_bsk.argtypes = ([C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int] +
                                               [C.c_uint32] * 4)
        libs.append(L)
    nbytes = libs[0].concrete_hip_fourier_bsk_size_bytes(p.n, p.k, p.level, p.N)
    out = torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream

    def one(L):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.concrete_hip_convert_bsk(s, 0, out.data_ptr(), key.ctypes.data, 0, p.n, p.k, p.level, p.N)
        torch.cuda.synchronize()
        assert rc == 0, rc
        return (time.perf_counter() - t0) * 1e3

    for L in libs:  # warm-up: code objects, the pool's first blocks
        one(L)
    times = [[] for _ in libs]
    for _ in range(reps):
        for i, L in enumerate(libs):
            times[i].append(one(L))
    print(f"concrete_hip_convert_bsk, cfg2 key (n={p.n} k={p.k} N={p.N} l={p.level}), host source, ms per call")
    for path, t in zip(paths, times):
        print(f"{path}: " + " ".join(f"{x:.3f}" for x in t) + f"  median {np.median(t):.3f}  max {max(t):.3f}")
    a, b = times
    ok = np.median(b) <= 1.05 * max(a)
    print(f"verdict: median of {paths[1]} {np.median(b):.3f} ms {'<=' if ok else '>'} 1.05 x slowest of "
          f"{paths[0]} {1.05 * max(a):.3f} ms: {'PASS' if ok else 'FAIL'}")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", nargs=2, metavar=("LIB_A", "LIB_B"))
    a = ap.parse_args()
    sys.exit(timing(a.time) if a.time else digests())
