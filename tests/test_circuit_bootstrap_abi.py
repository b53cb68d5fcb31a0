"""The circuit-bootstrap entry points (WoP-PBS stage 2) without a device: the declarations and
bindings, the support and scratch-size queries, the fp-ks key generator against tests/cbs_reference.py and against
decryption, the refusals made before the first device call (tests/c_client/circuit_bootstrap_client.c, as C99),
and the CPU reference checked against itself: the GGSWs it produces select, in a CMUX, the polynomial their bit
names."""
import os
import shutil
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

from concrete_amd import _native
from concrete_amd import backend as B

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cbs_reference as R  # noqa: E402
import vp_reference as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "concrete_amd")

NAMES = ("cuda_fp_keyswitch_lwe_to_glwe_64", "scratch_cuda_circuit_bootstrap_64", "cuda_circuit_bootstrap_64",
         "cleanup_cuda_circuit_bootstrap", "concrete_hip_fp_keyswitch", "concrete_hip_circuit_bootstrap",
         "concrete_hip_circuit_bootstrap_scratch_bytes", "concrete_hip_circuit_bootstrap_supported",
         "concrete_hip_fpksk_size_words", "concrete_hip_fpksk_generate")

P = B.PbsParams
# (BSK parameters, (level, base_log) of the fp-ks key, of the circuit bootstrap, supported)
SETS = [
    (P(620, 2, 1024, 3, 12), (2, 17), (2, 8), True),    # wop_pbs_2022-11-15_128: the 8-bit row
    (P(560, 2, 1024, 7, 6), (3, 13), (5, 5), True),     # the 16-bit row
    (P(8, 1, 512, 2, 10), (2, 15), (2, 10), True),
    (P(8, 1, 1024, 3, 7), (1, 40), (4, 8), True),       # an fp-ks digit beyond 32 bits
    (P(8, 1, 1024, 3, 9), (2, 15), (16, 3), True),      # a PBS on the general path's companion key; 16 cbs levels
    (P(8, 1, 1024, 2, 15), (4, 10), (1, 63), True),     # level_cbs * base_log_cbs = 63
    (P(8, 1, 1024, 3, 30), (2, 15), (2, 10), False),    # the PBS: level * base_log >= 64
    (P(8, 1, 1000, 3, 7), (2, 15), (2, 10), False),     # the PBS: no such polynomial size
    (P(8, 1, 1024, 3, 7), (4, 16), (2, 10), False),     # the fp-ks: level * base_log = 64
    (P(8, 1, 1024, 3, 7), (0, 15), (2, 10), False),     # the fp-ks: no level
    (P(8, 1, 1024, 3, 7), (2, 15), (0, 10), False),     # level_cbs = 0
    (P(8, 1, 1024, 3, 7), (2, 15), (8, 8), False),      # level_cbs * base_log_cbs = 64
]


def _conditions(p, pksk, cbs):
    """The four conditions of concrete_hip_circuit_bootstrap_supported, from the queries that already exist."""
    L = _native.lib()
    return (L.concrete_hip_pbs_supported(p.k, p.N, p.level, p.base_log) == 1 and
            L.concrete_hip_keyswitch_supported(pksk[0], pksk[1], p.k * p.N + 1, (p.k + 1) * p.N - 1) == 1 and
            cbs[0] >= 1 and cbs[0] * cbs[1] <= 63)


def test_symbols_are_declared_and_bound():
    declared = _native.declared_symbols()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/concrete_hip.h"
        assert name in _native.SIGNATURES, f"{name} has no ctypes signature"
        getattr(_native.lib(), name)
    assert _native.lib().concrete_hip_abi_version() == 5  # the capability is found through _supported
    for f in ("fpksk_generate", "fp_keyswitch", "circuit_bootstrap", "circuit_bootstrap_supported",
              "circuit_bootstrap_scratch_bytes"):
        assert callable(getattr(B, f))


@pytest.mark.parametrize("p,pksk,cbs,ok", SETS,
                         ids=[f"k{s[0].k}N{s[0].N}br{s[0].level}x{s[0].base_log}pp{s[1][0]}x{s[1][1]}cb{s[2][0]}x{s[2][1]}"
                              for s in SETS])
def test_supported_agrees_with_its_four_conditions(p, pksk, cbs, ok):
    assert _conditions(p, pksk, cbs) == ok
    assert B.circuit_bootstrap_supported(p, *pksk, *cbs) == ok


def test_both_outcomes_and_a_table_row_are_covered():
    assert {s[3] for s in SETS} == {True, False}
    assert any((s[0].k, s[0].N, s[0].level, s[0].base_log, s[1], s[2]) == (2, 1024, 3, 12, (2, 17), (2, 8)) for s in SETS)


def test_scratch_bytes_never_decrease():
    p = P(620, 2, 1024, 3, 12)

    def series(f, values):
        sizes = [f(v) for v in values]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        return sizes

    by_samples = series(lambda s: B.circuit_bootstrap_scratch_bytes(p, 2, s), (1, 2, 3, 16, 17, 80, 4096))
    series(lambda lv: B.circuit_bootstrap_scratch_bytes(p, lv, 5), range(1, 17))
    # the PBS input and output rows alone
    assert by_samples[-1] >= 4096 * 2 * 8 * (p.n + 1 + p.big_n + 1)
    assert B.circuit_bootstrap_scratch_bytes(p, 2, 0) == 0 and B.circuit_bootstrap_scratch_bytes(p, 0, 5) == 0
    assert B.circuit_bootstrap_scratch_bytes(replace(p, N=65536), 2, 5) == 0   # (k+1) N past the keyswitch's rows
    assert B.circuit_bootstrap_scratch_bytes(p, 2, 0xffffffff) == 0            # sizes that overflow


def test_fpksk_size_words():
    L = _native.lib()
    for k, N, level in [(1, 256, 2), (2, 1024, 2), (2, 1024, 3)]:
        assert L.concrete_hip_fpksk_size_words(k, N, level) == R.fpksk_words(k, N, level) == B.fpksk_words(k, N, level)
    # the optimizer's WoP rows: 302 MB at level 2, 453 MB at level 3
    assert 8 * R.fpksk_words(2, 1024, 2) == 8 * 3 * 2049 * 2 * 3072 == 302_137_344
    assert 8 * R.fpksk_words(2, 1024, 3) == 453_206_016
    assert L.concrete_hip_fpksk_size_words(0xffffffff, 0xffffffff, 0xffffffff) == 0


# ---------------------------------------------------------------------------------------------------------
# concrete_hip_fpksk_generate
# ---------------------------------------------------------------------------------------------------------
GK, GN, GLEVEL, GBASE = 1, 256, 2, 15
GSTD = 2.0 ** -40


@pytest.fixture(scope="module")
def genkey():
    from oracle import pyoracle as O
    O.lib()
    p = P(1, GK, GN, 1, 1)
    glwe_sk = O.binary_key(GK * GN, 9101)
    key = B.fpksk_generate(p, glwe_sk, GLEVEL, GBASE, 9102, std=GSTD)
    return dict(O=O, p=p, glwe_sk=glwe_sk, key=key)


def test_fpksk_generate_matches_the_reference(genkey):
    ref = R.fpksk_generate(genkey["glwe_sk"], GK, GN, GLEVEL, GBASE, GSTD, 9102)
    assert genkey["key"].shape == ref.shape == (GK + 1, GK * GN + 1, GLEVEL, (GK + 1) * GN)
    assert np.array_equal(genkey["key"], ref)


def test_fpksk_generate_is_deterministic_per_seed(genkey):
    again = B.fpksk_generate(genkey["p"], genkey["glwe_sk"], GLEVEL, GBASE, 9102, std=GSTD)
    other = B.fpksk_generate(genkey["p"], genkey["glwe_sk"], GLEVEL, GBASE, 9103, std=GSTD)
    assert np.array_equal(again, genkey["key"])
    assert not np.array_equal(other, genkey["key"])
    # every block has its own stream: no two blocks share their first mask word
    firsts = genkey["key"][:, :, 0, 0].reshape(-1)
    assert len(set(firsts.tolist())) == firsts.size


def test_fpksk_entries_decrypt_to_their_polynomials(genkey):
    """Entry (i, j, t) decrypts to -s_j 2^(64 - base_log (l - t)) P_i within the noise: a Gaussian of
    sigma = GSTD 2^64 = 2^24 per coefficient; 2^24 * 8 = 2^27 is eight sigma (none of the 1028 x 256 samples is
    expected past it: the two-sided tail is 1.2e-15 each)."""
    O, sk, key = genkey["O"], genkey["glwe_sk"], genkey["key"]
    L = O.lib()
    u64p = R.u64p
    L.ora_glwe_decrypt.argtypes = [u64p, u64p, u64p, R.sz, R.sz]
    L.ora_glwe_decrypt.restype = None
    mask = (1 << 64) - 1
    worst = 0
    for i in range(GK + 1):
        for j in range(GK * GN + 1):
            minus_s = (-int(sk[j])) & mask if j < GK * GN else 1
            for t in range(GLEVEL):
                factor = (minus_s << (64 - GBASE * (GLEVEL - t))) & mask
                want = np.zeros(GN, dtype=np.uint64)
                if i < GK:
                    want[:] = sk[i * GN:(i + 1) * GN] * np.uint64(factor)
                else:
                    want[0] = np.uint64((-factor) & mask)
                got = np.zeros(GN, dtype=np.uint64)
                L.ora_glwe_decrypt(O.P(sk), key[i, j, t].ctypes.data_as(u64p), O.P(got), GK, GN)
                err = (got - want).view(np.int64)
                worst = max(worst, int(np.abs(err).max()))
    assert 0 < worst <= 2 ** 27, worst


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not installed")
def test_c99_client_and_refusals_without_a_device(tmp_path):
    """The client compiles warning-free as C99 against the header and links the library; it then runs with
    every device hidden, so a refusal that reached a device call would abort instead of returning its code."""
    exe = tmp_path / "circuit_bootstrap_client"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_client", "circuit_bootstrap_client.c"), "-L", LIBDIR,
                    "-lconcrete_hip", f"-Wl,-rpath,{LIBDIR}", "-o", str(exe)], check=True)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "circuit_bootstrap_client ok" in out.stdout, out.stdout + out.stderr


def test_refusals_through_python():
    L = _native.lib()
    rc = L.concrete_hip_circuit_bootstrap(None, 0, 64, 64, 64, 64, 64, 620, 2, 1024, 3, 12, 2, 17, 2, 8, 3, None, 0,
                                          None)
    assert rc == -3
    with pytest.raises(RuntimeError, match="delta_log=64"):
        _native.check(rc, "concrete_hip_circuit_bootstrap")
    rc = L.concrete_hip_fp_keyswitch(None, 0, 64, 64, 64, 2048, 2, 1024, 17, 2, 3, 0)
    assert rc == -3
    with pytest.raises(RuntimeError, match="num_keys=0"):
        _native.check(rc, "concrete_hip_fp_keyswitch")


# ---------------------------------------------------------------------------------------------------------
# the reference against itself
# ---------------------------------------------------------------------------------------------------------
K, N, LWE_N = 1, 512, 8
BSK, PKSK, CBS = (2, 10), (2, 15), (2, 10)
KEY_STD = 2.0 ** -52
WIDTH = 2  # message bits, at the top of the word
BITS = (0, 1, 1, 0)


@pytest.fixture(scope="module")
def ref():
    from oracle import pyoracle as O
    O.lib()
    lwe_sk = O.binary_key(LWE_N, 9201)
    glwe_sk = O.binary_key(K * N, 9202)
    op = O.Params(n=LWE_N, k=K, N=N, l=BSK[0], logB=BSK[1])
    bsk = O.keygen_bsk(op, lwe_sk, glwe_sk, 9203, std=KEY_STD)
    fpksk = R.fpksk_generate(glwe_sk, K, N, PKSK[0], PKSK[1], KEY_STD, 9204)
    rng = np.random.RandomState(9205)
    table = rng.randint(0, 1 << WIDTH, size=(2, N)).astype(np.uint64)
    polys = np.zeros((2, (K + 1) * N), dtype=np.uint64)  # two trivial GLWEs
    polys[:, K * N:] = table << np.uint64(64 - WIDTH)
    return dict(O=O, lwe_sk=lwe_sk, glwe_sk=glwe_sk, bsk=bsk, fpksk=fpksk, table=table, polys=polys)


@pytest.mark.parametrize("delta_log", (63, 60))
def test_reference_composition_decrypts(ref, delta_log):
    """Bits 0/1/1/0 at delta_log, circuit-bootstrapped on the CPU, each GGSW put through vp_reference.cmux on two
    polynomials of 2-bit messages in the top bits: every output decrypts to the polynomial its bit selects.  The
    drift measured for this composition is 2^57 against the 2^61 half-window of a 2-bit message: four bits of
    room, asserted here as a drift below 2^59."""
    O = ref["O"]
    cts = O.lwe_encrypt_batch(ref["lwe_sk"], [b << delta_log for b in BITS], LWE_N, KEY_STD, 9300 + delta_log)
    ggsw, w = R.circuit_bootstrap(cts, ref["bsk"], ref["fpksk"], delta_log, LWE_N, K, N, *BSK, *PKSK, *CBS)
    assert ggsw.shape == (len(BITS), CBS[0], K + 1, (K + 1) * N) and w.shape == (len(BITS), CBS[0], K * N + 1)
    L = O.lib()
    L.ora_glwe_decrypt.argtypes = [R.u64p, R.u64p, R.u64p, R.sz, R.sz]
    L.ora_glwe_decrypt.restype = None
    worst = 0
    for s, bit in enumerate(BITS):
        G = ggsw[s].reshape(CBS[0], K + 1, K + 1, N)
        out = V.cmux(ref["polys"][0], ref["polys"][1], G, K, N, *CBS)
        dec = np.zeros(N, dtype=np.uint64)
        L.ora_glwe_decrypt(O.P(ref["glwe_sk"]), O.P(out), O.P(dec), K, N)
        want = ref["table"][bit]
        got = ((dec + np.uint64(1 << (63 - WIDTH))) >> np.uint64(64 - WIDTH)) % np.uint64(1 << WIDTH)
        assert np.array_equal(got, want), f"input {s} (bit {bit})"
        err = (dec - (want << np.uint64(64 - WIDTH))).view(np.int64)
        worst = max(worst, int(np.abs(err).max()))
    print(f"delta_log {delta_log}: worst drift 2^{np.log2(max(worst, 1)):.1f}")
    assert worst < 2 ** 59
