"""Timing of the vertical packing (concrete_hip_vertical_packing).

Shape: k = 1, N = 2048, level 3, base_log 8 (no WoP-PBS parameter row is recorded in the repository's fixtures).
Geometry: r = 6 tree GGSWs, mbr_size = 11 rotation GGSWs, tau = 5 outputs, 1 and 64 lookups.
Per lookup count three calls are timed, alternating inside one process, each repetition with device events
(a call includes its GGSW conversion and the gate's host synchronisation): the whole call (r, m), the tree alone
(r, 0) and the rotation alone (0, m).  At one lookup the rotation is also run by the PBS kernel the library already
had (concrete_hip_pbs with n = mbr_size on the synthetic LWE rows of tests/vp_reference.py, the GGSWs converted
once beforehand as a bootstrapping key); its output is compared word for word with the rotation call's first.
The GGSWs of the 64 lookups are those of the first, repeated at distinct addresses.
Informational: nothing gates on these numbers.

  python tools/vertical_packing_timing.py [--reps 5] [--lookups 1 64]      JSON lines
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from concrete_amd import backend as B  # noqa: E402
import vp_reference as V  # noqa: E402

DEV = "cuda:0"
K, N, LEVEL, BASE_LOG, R, M, TAU = 1, 2048, 3, 8, 6, 11, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lookups", type=int, nargs="+", default=[1, 64])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    from oracle import pyoracle as O
    p = B.PbsParams(n=M, k=K, N=N, level=LEVEL, base_log=BASE_LOG)
    assert B.vertical_packing_supported(p)
    rng = np.random.RandomState(11)
    bits = rng.randint(0, 2, size=(1, R + M))
    ggsws = V.ggsw_encrypt(O.binary_key(K * N, 12), bits, K, N, LEVEL, BASE_LOG, 2.0 ** -52, 13)
    luts = rng.randint(0, 16, size=(TAU, 1 << R, N)).astype(np.uint64) << np.uint64(60)
    d_luts = B.to_device(luts, DEV)
    d_one = B.to_device(ggsws.reshape(1, R + M, -1), DEV)

    for lookups in a.lookups:
        d_all = d_one.repeat(lookups, 1, 1).contiguous()
        d_tree = d_all[:, :R].contiguous()
        d_rot = d_all[:, R:].contiguous()
        scratch = torch.empty(B.vertical_packing_scratch_bytes(p, R, M, TAU, lookups) // 8, dtype=torch.int64, device=DEV)
        out = torch.empty((lookups, TAU, p.lwe_out_size), dtype=torch.int64, device=DEV)
        glwe = torch.empty((lookups, TAU, p.glwe_size), dtype=torch.int64, device=DEV)
        # the rotation alone starts from trivial GLWEs of the first LUT polynomials (same work per step)
        d_rot_luts = d_luts[:, :1].contiguous()

        def whole():
            return B.vertical_packing(p, d_all, d_luts, R, M, lookups, out=out, scratch=scratch)[0]

        def tree():
            return B.vertical_packing(p, d_tree, d_luts, R, 0, lookups, out=out, tree_out=glwe, scratch=scratch)[0]

        def rotation():
            return B.vertical_packing(p, d_rot, d_rot_luts, 0, M, lookups, out=out, scratch=scratch)[0]

        versions = {"whole": whole, "tree": tree, "rotation": rotation}
        equal = None
        if lookups == 1:
            fbsk = B.convert_bsk(p, V.pbs_key(ggsws[0, R:]), DEV)
            accs = B.to_device(np.stack([B.trivial_glwe(p, luts[o, 0]) for o in range(TAU)]), DEV)
            rows = B.to_device(np.tile(V.synthetic_lwe(M, N), (TAU, 1)), DEV)
            idx = B.to_device(np.arange(TAU, dtype=np.uint64), DEV)
            pbs_out = torch.empty((TAU, p.lwe_out_size), dtype=torch.int64, device=DEV)

            def rotation_pbs():
                return B.pbs(p, fbsk, rows, accs, lut_idx=idx, out=pbs_out)

            versions["rotation_by_concrete_hip_pbs"] = rotation_pbs
            equal = bool(torch.equal(rotation().clone()[0], rotation_pbs()))
            assert equal, "the rotation call and concrete_hip_pbs differ"
        for f in versions.values():  # warm-up of every shape
            f()
        torch.cuda.synchronize()
        assert B.stream_status(DEV) == 0
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
            print(json.dumps({"version": k, "k": K, "N": N, "level": LEVEL, "base_log": BASE_LOG, "r": R, "mbr_size": M,
                              "tau": TAU, "lookups": lookups, "ms_median": round(float(np.median(v)), 3),
                              "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "reps": a.reps,
                              "rotation_equals_pbs": equal if k.startswith("rotation") else None}), flush=True)


if __name__ == "__main__":
    main()
