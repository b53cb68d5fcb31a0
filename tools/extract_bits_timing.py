"""Timing of the fused bit extraction (concrete_hip_extract_bits) against the same work
composed in Python from the public keyswitch and PBS with torch elementwise steps.

Shape: full cfg2 (n = 630, k = 1, N = 1024), B = 4096 rows, number_of_bits = 4, delta_log = 60.
The two versions alternate inside one process, each repetition timed with device events; their outputs
are compared word for word first.  Informational: nothing gates on these numbers.

  python tools/extract_bits_timing.py [--batch 4096] [--bits 4] [--reps 5]        both versions, JSON lines
  rocprofv3 --kernel-trace --stats ... -- python tools/extract_bits_timing.py --fused-only --reps 2
                                                                                   per-kernel times
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from concrete_amd import backend as B  # noqa: E402

DEV = "cuda:0"


def composed(torch, p, fbsk, ksk_dev, d_in, nb, dl, accs):
    out = torch.empty((d_in.shape[0], nb, p.n + 1), dtype=torch.int64, device=DEV)
    c = d_in.clone()
    for t in range(nb):
        u = B.keyswitch(p, ksk_dev, c << (64 - dl - t - 1))
        out[:, nb - 1 - t] = u
        if t == nb - 1:
            break
        u[:, -1] += 1 << 62
        v = B.pbs(p, fbsk, u, accs[t:t + 1])
        v[:, -1] += 1 << (dl - 1 + t)
        c -= v
    return out.reshape(-1, p.n + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    p, nb, dl = B.CFG2, a.bits, 64 - a.bits
    lwe_sk, glwe_sk = B.binary_key(p.n, 1), B.binary_key(p.big_n, 2)
    fbsk = B.convert_bsk(p, B.bsk_generate(p, lwe_sk, glwe_sk, 3, std=2.0 ** -52), DEV)
    ksk_dev = B.to_device(B.ksk_generate(p, glwe_sk, lwe_sk, 4, std=2.0 ** -52), DEV)
    rng = np.random.RandomState(5)
    pts = (rng.randint(0, 1 << nb, size=a.batch).astype(np.uint64) << np.uint64(dl)) + np.uint64(1 << (dl - 3))
    d_in = B.to_device(B.lwe_encrypt(glwe_sk, pts, p.big_n, 2.0 ** -25, 6), DEV)
    accs = np.zeros((max(nb - 1, 1), p.glwe_size), dtype=np.uint64)
    for t in range(nb - 1):
        accs[t, p.k * p.N:] = np.uint64((-(1 << (dl - 1 + t))) & ((1 << 64) - 1))
    accs = B.to_device(accs, DEV)

    def fused():
        return B.extract_bits(p, fbsk, ksk_dev, d_in, nb, dl)

    def comp():
        return composed(torch, p, fbsk, ksk_dev, d_in, nb, dl, accs)

    versions = {"fused": fused} if a.fused_only else {"fused": fused, "composed": comp}
    outs = {k: f() for k, f in versions.items()}  # warm-up of every shape, and the outputs to compare
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    if not a.fused_only:
        assert torch.equal(outs["fused"], outs["composed"]), "fused and composed outputs differ"
    dec = B.lwe_decrypt(lwe_sk, B.to_host(outs["fused"][:4 * nb]), p.n)
    got = [((int(d) + (1 << 62)) >> 63) & 1 for d in dec]
    want = [(int(pt) >> (dl + nb - 1 - j)) & 1 for pt in pts[:4] for j in range(nb)]
    assert got == want, (got, want)
    times = {k: [] for k in versions}
    for _ in range(a.reps):
        for k, f in versions.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    for k, v in times.items():
        print(json.dumps({"version": k, "config": "cfg2", "batch": a.batch, "number_of_bits": nb, "delta_log": dl,
                          "ms_median": round(float(np.median(v)), 3), "ms_min": round(min(v), 3),
                          "ms_max": round(max(v), 3), "reps": a.reps,
                          "outputs_equal": None if a.fused_only else True}))


if __name__ == "__main__":
    main()
