"""The chained WoP-PBS entry points without a device: the declarations and bindings, the support
and scratch-size queries, the refusals made before the first device call, and the CPU reference chain
(tests/wop_reference.py) checked against decryption at the shapes tests/test_gpu_wop_pbs.py decrypts."""
import os
import subprocess
import sys
import textwrap
from dataclasses import replace

import numpy as np
import pytest

from concrete_amd import _native
from concrete_amd import backend as B
from concrete_amd import runtime as RT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_shapes as S  # noqa: E402
import wop_cases as Cs  # noqa: E402
import wop_reference as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("scratch_cuda_circuit_bootstrap_vertical_packing_64", "cuda_circuit_bootstrap_vertical_packing_64",
         "cleanup_cuda_circuit_bootstrap_vertical_packing", "scratch_cuda_wop_pbs_64", "cuda_wop_pbs_64",
         "cleanup_cuda_wop_pbs", "concrete_hip_circuit_bootstrap_vertical_packing", "concrete_hip_wop_pbs_crt",
         "concrete_hip_wop_pbs_scratch_bytes", "concrete_hip_wop_pbs_supported", "concrete_hip_keyset_add_fpksk",
         "memref_wop_pbs_crt_buffer_hip_u64", "memref_wop_pbs_crt_buffer_cuda_u64")

P = B.PbsParams
# (BSK and KS parameters, fp-ks (level, base_log), circuit bootstrap (level, base_log), supported)
SETS = [
    (Cs.P, Cs.PKSK, Cs.CBS, True),                                # shape A of the GPU tests
    (P(620, 2, 1024, 3, 12, 5, 3), (2, 17), (2, 8), True),        # the WoP table's ring
    (P(8, 1, 1024, 3, 9, 4, 3), (2, 15), (4, 5), True),           # a PBS on the general path's companion key
    (P(8, 1, 2048, 1, 23, 5, 3), (2, 15), (2, 8), True),
    (P(8, 1, 512, 2, 10, 8, 8), (2, 15), (4, 5), False),          # stage 1: keyswitch level * base_log = 64
    (P(8, 1, 512, 2, 32, 4, 4), (2, 15), (4, 5), False),          # stages 1 and 2: PBS level * base_log = 64
    (P(8, 1, 512, 2, 10, 4, 4), (4, 16), (4, 5), False),          # stage 2: fp-ks level * base_log = 64
    (P(8, 1, 512, 2, 10, 4, 4), (2, 15), (0, 5), False),          # stage 2: level_cbs = 0
    (P(8, 1, 512, 2, 10, 4, 4), (2, 15), (2, 30), False),         # stage 3 alone: digits the general path does not keep exact
    (P(8, 4, 512, 2, 10, 4, 4), (2, 15), (4, 5), False),          # stage 3 alone: k = 4
    (P(8, 1, 4096, 1, 22, 4, 4), (2, 15), (4, 5), False),         # stage 3 alone: N = 4096
]


def _conjunction(p, pksk, cbs):
    L = _native.lib()
    return (L.concrete_hip_extract_bits_supported(p.big_n, p.n, p.k, p.N, p.base_log, p.level, p.ks_base_log,
                                                  p.ks_level),
            L.concrete_hip_circuit_bootstrap_supported(p.k, p.N, p.level, p.base_log, pksk[0], pksk[1], cbs[0], cbs[1]),
            L.concrete_hip_vertical_packing_supported(p.k, p.N, cbs[0], cbs[1]))


def test_symbols_are_declared_and_bound():
    declared = _native.declared_symbols()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/concrete_hip.h"
        assert name in _native.SIGNATURES, f"{name} has no ctypes signature"
        getattr(_native.lib(), name)
    assert _native.lib().concrete_hip_abi_version() == 5  # the capability is found through _supported
    for f in ("wop_pbs_crt", "circuit_bootstrap_vertical_packing", "wop_pbs_supported", "wop_pbs_scratch_bytes",
              "crt_extract_bits"):
        assert callable(getattr(B, f))
    assert callable(RT.wop_pbs_crt) and callable(RT.Keyset.add_fpksk)


@pytest.mark.parametrize("p,pksk,cbs,ok", SETS, ids=[
    f"k{s[0].k}N{s[0].N}br{s[0].level}x{s[0].base_log}ks{s[0].ks_level}x{s[0].ks_base_log}pp{s[1][0]}x{s[1][1]}"
    f"cb{s[2][0]}x{s[2][1]}" for s in SETS])
def test_supported_is_the_conjunction_of_the_three_stages(p, pksk, cbs, ok):
    stages = _conjunction(p, pksk, cbs)
    assert all(v in (0, 1) for v in stages)
    assert (stages == (1, 1, 1)) == ok
    assert B.wop_pbs_supported(p, *pksk, *cbs) == ok


def test_every_stage_refuses_alone_somewhere():
    """The hand-picked sets hold both outcomes, and for each stage a set that only that stage refuses."""
    assert {s[3] for s in SETS} == {True, False}
    refusals = {_conjunction(*s[:3]) for s in SETS}
    assert {(0, 1, 1), (1, 0, 1), (1, 1, 0)} <= refusals


def test_supported_on_every_row_of_the_wop_table():
    assert len(S.WOP_ROWS) == 272
    for r in S.WOP_ROWS:
        p = P(r["n"], r["k"], r["N"], r["br_l"], r["br_b"], r["ks_l"], r["ks_b"])
        assert B.wop_pbs_supported(p, r["pp_l"], r["pp_b"], r["cb_l"], r["cb_b"]), r


def test_scratch_bytes_never_decrease():
    p = P(620, 2, 1024, 3, 12, 5, 3)

    def series(f, values):
        sizes = [f(v) for v in values]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        return sizes

    for blocks in (0, 3):  # without and with stage 1
        series(lambda b: B.wop_pbs_scratch_bytes(p, 2, blocks, 12, 3, b), (1, 2, 3, 16, 17, 64, 65))
        by_t = series(lambda t: B.wop_pbs_scratch_bytes(p, 2, blocks, t, 3, 2), range(3, 21))  # log2 N = 10 inside
        series(lambda tau: B.wop_pbs_scratch_bytes(p, 2, blocks, 9, tau, 2), (1, 2, 3, 4, 5, 8, 9, 16, 33))
        series(lambda lv: B.wop_pbs_scratch_bytes(p, lv, blocks, 12, 3, 2), range(1, 17))
        assert all(s % 16 == 0 for s in by_t)
    # the GGSWs alone: batch x t x level_cbs x (k+1) x (k+1) N words
    assert B.wop_pbs_scratch_bytes(p, 2, 3, 12, 3, 2) >= 8 * 2 * 12 * 2 * 3 * 3 * 1024
    # a chain with stage 1 needs no less than one without
    assert B.wop_pbs_scratch_bytes(p, 2, 3, 12, 3, 2) >= B.wop_pbs_scratch_bytes(p, 2, 0, 12, 3, 2)
    zero = [B.wop_pbs_scratch_bytes(p, 2, 3, 0, 3, 2), B.wop_pbs_scratch_bytes(p, 2, 3, 12, 0, 2),
            B.wop_pbs_scratch_bytes(p, 2, 3, 12, 3, 0), B.wop_pbs_scratch_bytes(p, 0, 3, 12, 3, 2),
            B.wop_pbs_scratch_bytes(p, 2, 13, 12, 3, 2),             # more blocks than bits
            B.wop_pbs_scratch_bytes(p, 2, 3, 10 + 25, 3, 2),         # a tree deeper than 24
            B.wop_pbs_scratch_bytes(replace(p, N=1000), 2, 3, 12, 3, 2),
            B.wop_pbs_scratch_bytes(p, 2, 3, 12, 3, 0xffffffff),     # sizes that overflow
            B.wop_pbs_scratch_bytes(p, 2, 3, 30, 0xffffffff, 2)]
    assert zero == [0] * len(zero)


REFUSALS = textwrap.dedent("""
    import ctypes as C
    import numpy as np
    from concrete_amd import _native
    L = _native.lib()
    err = lambda: L.concrete_hip_last_error().decode()
    mods = np.array([3, 4, 5] + [2] * 14, dtype=np.uint64)
    m = mods.ctypes.data
    X = 64  # a non-null pointer no refused call may follow
    shape = (8, 1, 512, 2, 10, 4, 4, 2, 15, 4, 5)  # n, k, N, BSK, KS, fp-ks, CBS (level, base_log) each

    def crt(out=X, inp=X, luts=X, bsk=X, ksk=X, fpksk=X, moduli=m, blocks=3, batch=1, shape=shape, scratch=None,
            nbytes=0):
        return L.concrete_hip_wop_pbs_crt(None, 0, out, inp, luts, bsk, ksk, fpksk, moduli, blocks, batch, *shape,
                                          scratch, nbytes, None)

    def cbvp(out=X, inp=X, luts=X, bsk=X, fpksk=X, shape=(8, 1, 512, 2, 10, 2, 15, 4, 5), t=7, tau=3, lookups=1,
             scratch=None, nbytes=0):
        return L.concrete_hip_circuit_bootstrap_vertical_packing(None, 0, out, inp, luts, bsk, fpksk, *shape, t, tau,
                                                                 lookups, scratch, nbytes, None)

    for name in ("out", "inp", "luts", "bsk", "ksk", "fpksk", "moduli"):
        assert crt(**{name: None}) == -1 and "null pointer" in err(), name
    for name in ("out", "inp", "luts", "bsk", "fpksk"):
        assert cbvp(**{name: None}) == -1 and "null pointer" in err(), name
    assert crt(blocks=17) == -3 and "num_blocks=17" in err()            # more CRT blocks than the cap
    assert crt(blocks=16, batch=0) == 0                                 # the cap itself passes; nothing to do
    assert crt(blocks=0) == -3 and "num_blocks=0" in err()
    bad = mods.copy(); bad[1] = 1
    assert crt(moduli=bad.ctypes.data) == -3 and "modulus 1 is 1" in err()
    bad[1] = (1 << 63) + 1
    assert crt(moduli=bad.ctypes.data) == -3 and "modulus 1" in err()
    big = np.array([1 << 12] * 3, dtype=np.uint64)                      # t = 36 > log2 N + 24
    assert crt(moduli=big.ctypes.data) == -3 and "overflow" in err()
    assert cbvp(t=0) == -3 and cbvp(tau=0) == -3 and cbvp(t=34) == -3
    assert crt(batch=0xffffffff) == -3 and "overflow" in err()
    need = L.concrete_hip_wop_pbs_scratch_bytes(8, 1, 512, 4, 3, 7, 3, 1)
    assert need > 0 and need % 16 == 0
    assert crt(scratch=4096, nbytes=need - 16) == -3 and "scratch" in err()
    assert crt(scratch=4096 + 8, nbytes=need) == -3 and "scratch" in err()  # misaligned
    unsupported = (8, 1, 512, 2, 10, 8, 8, 2, 15, 4, 5)                 # keyswitch level * base_log = 64
    assert crt(shape=unsupported) == -2 and "unsupported parameters" in err()
    assert cbvp(shape=(8, 1, 512, 2, 10, 2, 15, 2, 30)) == -2 and "unsupported parameters" in err()
    # the keyset takes an fp-ks key list without a device, and refuses what the fp-ks would
    ks = L.concrete_hip_keyset_create()
    key = np.zeros(L.concrete_hip_fpksk_size_words(1, 256, 2), dtype=np.uint64)
    assert L.concrete_hip_keyset_add_fpksk(ks, 0, key.ctypes.data, 2, 15, 256, 1, 256) == 0
    assert L.concrete_hip_keyset_add_fpksk(ks, 1, key.ctypes.data, 2, 15, 255, 1, 256) == -3
    assert L.concrete_hip_keyset_add_fpksk(ks, 1, None, 2, 15, 256, 1, 256) == -3
    assert L.concrete_hip_keyset_add_fpksk(ks, 1, key.ctypes.data, 4, 16, 256, 1, 256) == -2
    L.concrete_hip_keyset_destroy(ks)
    print("wop refusals ok")
""")


def test_refusals_come_before_the_first_device_call():
    """Every -1 and -3 (and the parameter -2) of the two compute calls, in a process that sees no device: a refusal
    that reached a device call would abort instead of returning its code."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", REFUSALS], capture_output=True, text=True, timeout=120, env=env,
                         cwd=ROOT)
    assert out.returncode == 0 and "wop refusals ok" in out.stdout, out.stdout + out.stderr


def test_lut_layout_and_selected_index():
    luts = np.arange(3 * 8, dtype=np.uint64).reshape(3, 8)
    padded = W.lut_layout(luts, 3, 512)
    assert padded.shape == (3, 1, 512) and np.array_equal(padded[:, 0, :8], luts) and not padded[:, 0, 8:].any()
    big = np.arange(2 * 2048, dtype=np.uint64).reshape(2, 2048)
    assert np.array_equal(W.lut_layout(big, 11, 512), big.reshape(2, 4, 512))
    assert W.rm(7, 512) == (0, 7) and W.rm(9, 512) == (0, 9) and W.rm(13, 512) == (4, 9)
    # [3, 4, 5], value 2 * 20 + 3 * 15 + 4 * 12 mod 60 has residues (2, 3, 4): top bits floor(r 2^nb / m) = 2, 3, 6
    v = (2 * 40 + 3 * 45 + 4 * 36) % 60
    assert (v % 3, v % 4, v % 5) == (2, 3, 4)
    assert W.selected_index(v, (3, 4, 5)) == (6 << 4) | (3 << 2) | 2
    assert [W.crt_offset(nb) for nb in (3, 59, 60)] == [(1 << 60) - (1 << 56), (1 << 4) - 1, 1 << 3]


@pytest.mark.parametrize("moduli", Cs.MODULI_SETS, ids=lambda m: "x".join(map(str, m)))
def test_reference_chain_decrypts_with_margin(moduli):
    """The CPU chain at shape A: every output of every value decrypts to the table entry its CRT bits select, with a
    phase error of at most a quarter of the 2^61 half-window of a 2-bit message.  The device's words equal these
    (tests/test_gpu_wop_pbs.py), so this settles the GPU tests' decryption.  Measured: 2^57.1 to 2^57.8."""
    c = Cs.case(moduli)
    nblk = len(moduli)
    assert c["t"] == sum(W.crt_bits(m) for m in moduli) and c["values"][0] == 0
    phases = Cs.decrypt(c["want"].reshape(-1, Cs.K * Cs.N + 1))
    want = np.array([[int(c["table"][o, c["index"][b]]) for o in range(nblk)] for b in range(Cs.BATCH)]).reshape(-1)
    assert Cs.messages(phases) == want.tolist()
    err = (phases - (want.astype(np.uint64) << np.uint64(64 - Cs.WIDTH))).view(np.int64)
    worst = int(np.abs(err).max())
    print(f"{moduli}: worst phase error 2^{np.log2(max(worst, 1)):.2f}")
    assert worst <= (1 << 61) // 4
