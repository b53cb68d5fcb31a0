"""Timing of the chained WoP-PBS (concrete_hip_wop_pbs_crt) at the optimizer's WoP ring.

The 8-bit row of the WoP table at log norm2 = 0 (tests/golden/wop_pbs_last_128_rows.json: k = 2, N = 1024, n = 712,
br (2, 15), ks (7, 2), pp (2, 16), cb (2, 7)), two CRT decompositions, (4, 8, 8) (t = 8 < log2 N: the LUT layout
kernel runs, no tree) and (16, 16, 16) (t = 12: r = 2, m = 10), batches 1 and 64.  Per point five versions are timed
with device events, alternating inside one process:
  chained      one concrete_hip_wop_pbs_crt call on the caller's scratch
  composition  the same work as three public stage calls driven from Python (backend.crt_extract_bits, with its
               host-built offset vector uploaded per call, then circuit_bootstrap, then vertical_packing on a LUT
               laid out ahead of time)
  stage1 / stage2 / stage3   each of those three calls alone, on the buffers the composition left
The two outputs are compared word for word first.  The bootstrapping and keyswitch keys are real ones (the calls
are gated on the key's spectrum); the fp-ks key is random words.  Informational: nothing gates on these numbers.

  python tools/wop_chain_time.py [--reps 5] [--batches 1 64]      JSON lines
  python tools/wop_chain_time.py --chain-only 20 --batches 64     the chained call alone (for a kernel trace)
  python tools/wop_chain_time.py --kernel-stats stats.csv         JSON lines from a rocprofv3 --kernel-trace --stats
                                                                  CSV of such a run: the two new kernels' share
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from concrete_amd import backend as B  # noqa: E402

DEV = "cuda:0"
MODULI = ((4, 8, 8), (16, 16, 16))
NEW_KERNELS = ("wop_front_kernel", "wop_lut_pad_kernel")


def table_row(bits=8):
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "wop_pbs_last_128_rows.json")))["rows"]
    return next(r for r in rows if r["bits"] == bits and r["log_norm2"] == 0)


def kernel_stats(path):
    rows = list(csv.DictReader(open(path)))
    name = next(c for c in rows[0] if c.lower() in ("name", "kernelname", "kernel_name"))
    total = next(c for c in rows[0] if c.lower() in ("totaldurationns", "total_duration_ns", "totalduration(ns)"))
    calls = next(c for c in rows[0] if c.lower() in ("calls", "count"))
    whole = sum(float(r[total]) for r in rows)
    for r in rows:
        if any(k in r[name] for k in NEW_KERNELS):
            print(json.dumps({"kernel": r[name].split("(")[0], "calls": int(r[calls]),
                              "us_per_call": round(float(r[total]) / int(r[calls]) / 1e3, 2),
                              "share_of_kernel_time": round(float(r[total]) / whole, 6)}))
    print(json.dumps({"kernel_time_ms_total": round(whole / 1e6, 3), "kernels": len(rows)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--chain-only", type=int, default=0)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    r = table_row()
    p = B.PbsParams(n=r["n"], k=r["k"], N=r["N"], level=r["br_l"], base_log=r["br_b"], ks_level=r["ks_l"],
                    ks_base_log=r["ks_b"])
    (pl, pb), (cl, cb) = (r["pp_l"], r["pp_b"]), (r["cb_l"], r["cb_b"])
    assert B.wop_pbs_supported(p, pl, pb, cl, cb)
    lwe_sk, glwe_sk = B.binary_key(p.n, 31), B.binary_key(p.big_n, 32)
    fbsk = B.convert_bsk(p, B.bsk_generate(p, lwe_sk, glwe_sk, 33), DEV)
    d_ksk = B.to_device(B.ksk_generate(p, glwe_sk, lwe_sk, 34), DEV)
    key_words = B.fpksk_words(p.k, p.N, pl)
    gen = torch.Generator(device=DEV).manual_seed(35)
    d_fpksk = torch.randint(0, 1 << 32, (key_words,), dtype=torch.int64, device=DEV, generator=gen) << 32
    d_fpksk |= torch.randint(0, 1 << 32, (key_words,), dtype=torch.int64, device=DEV, generator=gen)
    vp = B.PbsParams(n=1, k=p.k, N=p.N, level=cl, base_log=cb)
    logn = p.N.bit_length() - 1
    for moduli in MODULI:
        nblk = len(moduli)
        t = sum(B.crt_bits(m) for m in moduli)
        rr, m = max(t - logn, 0), min(t, logn)
        rng = np.random.RandomState(36 + t)
        luts = rng.randint(0, 4, size=(nblk, 1 << t)).astype(np.uint64) << np.uint64(62)
        laid = np.zeros((nblk, 1 << rr, p.N), dtype=np.uint64)
        if t >= logn:
            laid[:] = luts.reshape(nblk, 1 << rr, p.N)
        else:
            laid[:, 0, :1 << t] = luts
        d_luts, d_laid = B.to_device(luts, DEV), B.to_device(laid, DEV)
        for batch in a.batches:
            values = rng.randint(0, int(np.prod(moduli)), size=batch)
            pts = np.array([B.crt_encode(v, q) for v in values for q in moduli], dtype=np.uint64)
            d_in = B.to_device(B.lwe_encrypt(glwe_sk, pts, p.big_n, B.secure_std(p.k, p.N), 37).reshape(
                batch, nblk, p.big_n + 1), DEV)
            out = torch.empty((batch, nblk, p.lwe_out_size), dtype=torch.int64, device=DEV)
            scratch = torch.empty(B.wop_pbs_scratch_bytes(p, cl, nblk, t, nblk, batch) // 8, dtype=torch.int64,
                                  device=DEV)
            state = {}

            def chained():
                return B.wop_pbs_crt(p, fbsk, d_ksk, d_fpksk, d_in, d_luts, moduli, pl, pb, cl, cb, out=out,
                                     scratch=scratch)[0]

            def stage1():
                state["bits"] = B.crt_extract_bits(p, fbsk, d_ksk, d_in, moduli).reshape(batch * t, p.n + 1)
                return state["bits"]

            def stage2():
                state["ggsw"] = B.circuit_bootstrap(p, fbsk, d_fpksk, state["bits"], 63, pl, pb, cl, cb)
                return state["ggsw"]

            def stage3():
                state["lwe"] = B.vertical_packing(vp, state["ggsw"].reshape(-1), d_laid, rr, m, batch)[0]
                return state["lwe"]

            def composition():
                stage1(), stage2()
                return stage3()

            if a.chain_only:
                for _ in range(a.chain_only):
                    chained()
                torch.cuda.synchronize()
                continue
            versions = {"chained": chained, "composition": composition, "stage1": stage1, "stage2": stage2,
                        "stage3": stage3}
            for f in versions.values():  # warm-up of every shape
                f()
            torch.cuda.synchronize()
            assert B.stream_status(DEV) == 0
            equal = bool(torch.equal(out, state["lwe"]))
            assert equal, "the chained call and the composition differ"
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
                print(json.dumps({"version": k, "moduli": list(moduli), "t": t, "r": rr, "m": m, "batch": batch,
                                  "k": p.k, "N": p.N, "n": p.n, "br": [p.level, p.base_log],
                                  "ks": [p.ks_level, p.ks_base_log], "pp": [pl, pb], "cb": [cl, cb],
                                  "ms_median": round(float(np.median(v)), 3), "ms_min": round(min(v), 3),
                                  "ms_max": round(max(v), 3), "reps": a.reps, "outputs_equal": equal}), flush=True)
            del scratch, state


if __name__ == "__main__":
    main()
