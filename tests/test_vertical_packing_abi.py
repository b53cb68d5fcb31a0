"""The vertical-packing entry points (WoP-PBS stage 3) without a device: the declarations and
bindings, the support and scratch-size queries, the refusals concrete_hip_vertical_packing makes before its first
device call (tests/c_client/vertical_packing_client.c, as C99), and the CPU reference of tests/vp_reference.py
checked against itself: what it computes decrypts to the LUT entry the GGSW bits select."""
import itertools
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
import vp_reference as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "concrete_amd")

NAMES = ("scratch_cuda_cmux_tree_64", "cuda_cmux_tree_64", "cleanup_cuda_cmux_tree",
         "scratch_cuda_blind_rotation_sample_extraction_64", "cuda_blind_rotate_and_sample_extraction_64",
         "cleanup_cuda_blind_rotation_sample_extraction", "concrete_hip_vertical_packing",
         "concrete_hip_vertical_packing_scratch_bytes", "concrete_hip_vertical_packing_supported")

P = B.PbsParams  # (n is not used by vertical packing)
# (parameters, whether the general path's gate generic_pbs_ok accepts (k, N, level, base_log))
SETS = [(P(1, 1, 512, 2, 10), True), (P(1, 1, 1024, 3, 8), True), (P(1, 1, 2048, 2, 12), True),
        (P(1, 2, 512, 2, 10), True), (P(1, 1, 1024, 2, 15), True), (P(1, 3, 1024, 1, 20), True),
        (P(1, 1, 1024, 3, 7), True),
        (P(1, 1, 1024, 3, 40), False),    # level * base_log > 64
        (P(1, 1, 1024, 1, 64), False),    # a 64-bit digit: five sub-digits, bound past the gate
        (P(1, 1, 1024, 0, 8), False)]     # no level


def test_symbols_are_declared_and_bound():
    declared = _native.declared_symbols()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/concrete_hip.h"
        assert name in _native.SIGNATURES, f"{name} has no ctypes signature"
        getattr(_native.lib(), name)
    assert _native.lib().concrete_hip_abi_version() == 5  # the capability is found through _supported
    for f in ("vertical_packing_supported", "vertical_packing_scratch_bytes", "vertical_packing"):
        assert callable(getattr(B, f))


@pytest.mark.parametrize("p,ok", SETS, ids=lambda v: f"k{v.k}N{v.N}l{v.level}b{v.base_log}" if isinstance(v, P) else None)
def test_supported_agrees_with_the_general_gate(p, ok):
    assert V.generic_pbs_ok(p.k, p.N, p.level, p.base_log) == ok
    assert B.vertical_packing_supported(p) == ok
    # outside the instantiated rings and GLWE dimensions the answer is no, whatever the gate says
    assert not B.vertical_packing_supported(replace(p, N=4096))
    assert not B.vertical_packing_supported(replace(p, N=1000))
    assert not B.vertical_packing_supported(replace(p, k=4))
    assert not B.vertical_packing_supported(replace(p, k=0))


def test_both_outcomes_are_covered():
    assert {ok for _, ok in SETS} == {True, False}


@pytest.mark.parametrize("p", [s for s, ok in SETS if ok][:5], ids=lambda p: f"k{p.k}N{p.N}l{p.level}")
def test_scratch_bytes_never_decrease(p):
    def series(f, values):
        sizes = [f(v) for v in values]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        return sizes

    series(lambda r: B.vertical_packing_scratch_bytes(p, r, 4, 3, 2), range(0, 13))
    series(lambda tau: B.vertical_packing_scratch_bytes(p, 3, 4, tau, 2), (1, 2, 3, 5, 64, 65))
    by_lookups = series(lambda n: B.vertical_packing_scratch_bytes(p, 3, 4, 3, n), (1, 2, 3, 64, 65, 4096))
    # the converted GGSWs and one GLWE per output alone
    assert by_lookups[-1] >= 4096 * (7 * L_key_bytes(p) + 3 * p.glwe_size * 8)
    series(lambda m: B.vertical_packing_scratch_bytes(p, 3, m, 3, 2), range(0, p.N.bit_length()))
    assert B.vertical_packing_scratch_bytes(p, 3, 4, 0, 2) == 0 and B.vertical_packing_scratch_bytes(p, 3, 4, 3, 0) == 0
    assert B.vertical_packing_scratch_bytes(p, 25, 4, 3, 2) == 0
    assert B.vertical_packing_scratch_bytes(p, 3, p.N.bit_length(), 3, 2) == 0  # mbr_size > log2 N


def L_key_bytes(p):
    return int(_native.lib().concrete_hip_generic_bsk_size_bytes(1, p.k, p.level, p.N))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not installed")
def test_c99_client_and_refusals_without_a_device(tmp_path):
    """The client compiles warning-free as C99 against the header and links the library; it then runs with
    every device hidden, so a refusal that reached a device call would abort instead of returning its code."""
    exe = tmp_path / "vertical_packing_client"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_client", "vertical_packing_client.c"), "-L", LIBDIR,
                    "-lconcrete_hip", f"-Wl,-rpath,{LIBDIR}", "-o", str(exe)], check=True)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "vertical_packing_client ok" in out.stdout, out.stdout + out.stderr


def test_refusals_through_python():
    L = _native.lib()
    rc = L.concrete_hip_vertical_packing(None, 0, 64, None, 64, 64, 1, 1024, 8, 3, 3, 4, 0, 1, None, 0, None, None)
    assert rc == -3
    with pytest.raises(RuntimeError, match="tau=0"):
        _native.check(rc, "concrete_hip_vertical_packing")


# ---------------------------------------------------------------------------------------------------------
# the reference against itself
# ---------------------------------------------------------------------------------------------------------
K, N, LEVEL, BASE_LOG, R, M, TAU = 1, 256, 3, 8, 2, 2, 2
KEY_STD = 2.0 ** -52
WIDTH = 4  # message bits, at the top of the word


@pytest.fixture(scope="module")
def ref():
    from oracle import pyoracle as O
    O.lib()
    rng = np.random.RandomState(4190)
    glwe_sk = O.binary_key(K * N, 4191)
    # every coefficient a 4-bit message in the top 4 bits
    table = rng.randint(0, 1 << WIDTH, size=(TAU, 1 << R, N)).astype(np.uint64)
    luts = table << np.uint64(64 - WIDTH)
    return dict(O=O, glwe_sk=glwe_sk, table=table, luts=luts)


def test_reference_drift_budget():
    """Worst case per CMUX and output coefficient: the (k+1) N level rounding terms of the decomposition, each
    at most 2^(63 - level * base_log) in magnitude times a key bit, plus the body's own; over the r + m
    CMUXes of a path that is (r + m)(kN + 1) 2^(63 - level * base_log).  It must stay under half the window
    2^60 that a 4-bit message in the top bits leaves (the GGSW noise 2^-52 * 2^64 = 2^12 per digit product is
    far below it)."""
    drift = (R + M) * (K * N + 1) * 2 ** (63 - LEVEL * BASE_LOG)
    assert drift < 2 ** 60 / 2


@pytest.mark.parametrize("pattern", list(itertools.product((0, 1), repeat=R + M)), ids=lambda b: "".join(map(str, b)))
def test_reference_decrypts_to_the_selected_entry(ref, pattern):
    O = ref["O"]
    ggsws = V.ggsw_encrypt(ref["glwe_sk"], np.array([pattern]), K, N, LEVEL, BASE_LOG, KEY_STD,
                           5000 + int("".join(map(str, pattern)), 2) * 16)
    lwe, glwe = V.vertical_packing(ggsws, ref["luts"], R, M, K, N, LEVEL, BASE_LOG)
    pi, ci = V.selected(ref["luts"], pattern[:R], pattern[R:])
    dec = O.lwe_decrypt_batch(ref["glwe_sk"], lwe[0], K * N)
    got = [int((int(d) + (1 << (63 - WIDTH))) >> (64 - WIDTH)) % (1 << WIDTH) for d in dec]
    assert got == [int(ref["table"][o, pi, ci]) for o in range(TAU)]
    # the drift actually seen stays inside the budget of test_reference_drift_budget
    budget = (R + M) * (K * N + 1) * 2 ** (63 - LEVEL * BASE_LOG)
    for o, d in enumerate(dec):
        err = (int(d) - (int(ref["table"][o, pi, ci]) << (64 - WIDTH))) % (1 << 64)
        assert min(err, (1 << 64) - err) <= budget
    # the rotation written out with ora_monomial_div is the rotation run as a PBS
    direct = V.sample_extract(V.rotate_direct(glwe[0], ggsws[0, R:], K, N, LEVEL, BASE_LOG), K, N)
    assert np.array_equal(direct, lwe[0])
