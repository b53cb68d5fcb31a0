"""Timing of the circuit bootstrap (concrete_hip_circuit_bootstrap).

Two rows of the optimizer's WoP table (compilers/concrete-optimizer/v0-parameters/ref/wop_pbs_2022-11-15_128 in
the reference), both k = 2, N = 1024:
  8-bit   n = 620, br (3, 12), cb (2, 8), pp (2, 17), 8 inputs:  16 PBS / fp-ks rows
  16-bit  n = 560, br (7, 6),  cb (5, 5), pp (3, 13), 16 inputs: 80 rows
Per point four calls are timed, alternating inside one process, each repetition with device events: the whole
call; its PBS part (concrete_hip_pbs on as many rows, the same key and accumulator count); its fp-ks part
(concrete_hip_fp_keyswitch on as many rows, k + 1 keys); and the comparison point, the library's LWE keyswitch on
the zero-padded rows (k + 1 calls of concrete_hip_keyswitch with n_in = kN + 1, n_out + 1 = (k+1)N, one per key),
which computes the same words: the two outputs are compared word for word first.  The bootstrapping key is a
real one (the calls are gated on its spectrum); the fp-ks key is random words (the map is linear in them).
Informational: nothing gates on these numbers.

  python tools/circuit_bootstrap_timing.py [--reps 5] [--points 8 16]      JSON lines
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from concrete_amd import _native  # noqa: E402
from concrete_amd import backend as B  # noqa: E402

DEV = "cuda:0"
K, N = 2, 1024
# bits: (n, br, cb, pp, inputs)
POINTS = {8: (620, (3, 12), (2, 8), (2, 17), 8), 16: (560, (7, 6), (5, 5), (3, 13), 16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, nargs="+", default=[8, 16])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    L = _native.lib()
    for bits in a.points:
        n, (bl, bb), (cl, cb), (pl, pb), inputs = POINTS[bits]
        p = B.PbsParams(n=n, k=K, N=N, level=bl, base_log=bb)
        assert B.circuit_bootstrap_supported(p, pl, pb, cl, cb)
        rows, W, G = inputs * cl, K * N + 1, (K + 1) * N
        lwe_sk, glwe_sk = B.binary_key(n, 21), B.binary_key(K * N, 22)
        fbsk = B.convert_bsk(p, B.bsk_generate(p, lwe_sk, glwe_sk, 23), DEV)
        key_words = B.fpksk_words(K, N, pl)
        gen = torch.Generator(device=DEV).manual_seed(24)
        d_key = torch.randint(0, 1 << 32, (key_words,), dtype=torch.int64, device=DEV, generator=gen) << 32
        d_key |= torch.randint(0, 1 << 32, (key_words,), dtype=torch.int64, device=DEV, generator=gen)
        cts = B.lwe_encrypt(lwe_sk, [(i & 1) << 63 for i in range(inputs)], n, B.secure_std(1, n), 25)
        d_in = B.to_device(cts, DEV)
        ggsw = torch.empty((inputs, cl, K + 1, G), dtype=torch.int64, device=DEV)
        w = torch.empty((inputs, cl, W), dtype=torch.int64, device=DEV)
        scratch = torch.empty(B.circuit_bootstrap_scratch_bytes(p, cl, inputs) // 8, dtype=torch.int64, device=DEV)

        def whole():
            return B.circuit_bootstrap(p, fbsk, d_key, d_in, 63, pl, pb, cl, cb, out=ggsw, scratch=scratch, pbs_out=w)

        whole()
        torch.cuda.synchronize()
        assert B.stream_status(DEV) == 0
        d_rows = w.reshape(rows, W).clone()  # what the fp-ks of the whole call read
        # the PBS part: as many rows, the same key, cl accumulators
        d_pbs_in = d_in.repeat_interleave(cl, dim=0).contiguous()
        accs = np.zeros((cl, G), dtype=np.uint64)
        for v in range(cl):
            accs[v, K * N:] = np.uint64((-(1 << (63 - cb * (v + 1)))) & ((1 << 64) - 1))
        d_accs = B.to_device(accs, DEV)
        d_idx = B.to_device(np.tile(np.arange(cl, dtype=np.uint64), inputs), DEV)
        pbs_out = torch.empty((rows, W), dtype=torch.int64, device=DEV)
        fp_out = torch.empty((rows, K + 1, G), dtype=torch.int64, device=DEV)
        # the comparison point: zero-padded rows through the LWE keyswitch, one call per key
        d_pad = torch.zeros((rows, W + 1), dtype=torch.int64, device=DEV)
        d_pad[:, :W] = d_rows
        ks_out = torch.empty((K + 1, rows, G), dtype=torch.int64, device=DEV)
        per_key = key_words // (K + 1)

        def pbs():
            return B.pbs(p, fbsk, d_pbs_in, d_accs, lut_idx=d_idx, out=pbs_out)

        def fpks():
            return B.fp_keyswitch(K, N, pl, pb, d_key, d_rows, out=fp_out)

        def lwe_keyswitch():
            for i in range(K + 1):
                _native.check(L.concrete_hip_keyswitch(B._stream(DEV), 0, ks_out[i].data_ptr(), None, d_pad.data_ptr(),
                                                       None, d_key.data_ptr() + 8 * i * per_key, W, G - 1, pb, pl, rows),
                              "concrete_hip_keyswitch")
            return ks_out

        versions = {"whole": whole, "pbs": pbs, "fp_keyswitch": fpks, "lwe_keyswitch_composition": lwe_keyswitch}
        for f in versions.values():  # warm-up of every shape
            f()
        torch.cuda.synchronize()
        assert B.stream_status(DEV) == 0
        equal = bool(torch.equal(fp_out, ks_out.permute(1, 0, 2))) and bool(torch.equal(fp_out.reshape(-1), ggsw.reshape(-1)))
        assert equal, "the fp-ks, the LWE keyswitch composition and the whole call differ"
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
            med = float(np.median(v))
            rec = {"version": k, "bits": bits, "k": K, "N": N, "n": n, "br": [bl, bb], "cb": [cl, cb], "pp": [pl, pb],
                   "inputs": inputs, "rows": rows, "ms_median": round(med, 3), "ms_min": round(min(v), 3),
                   "ms_max": round(max(v), 3), "reps": a.reps, "outputs_equal": equal}
            if k in ("fp_keyswitch", "lwe_keyswitch_composition"):
                rec["key_mb"] = round(8 * key_words / 1e6, 1)
                rec["key_gb_per_s"] = round(8 * key_words / (med * 1e-3) / 1e9, 1)
            print(json.dumps(rec), flush=True)
        del d_key, fbsk


if __name__ == "__main__":
    main()
