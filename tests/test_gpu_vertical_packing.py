"""GPU tests of the vertical packing (WoP-PBS stage 3; concrete_amd/csrc/vertical_packing.hip and
gen_cmux_kernel in pbs_generic.hip).

The definition is tests/vp_reference.py: a CMUX tree over r run-time GGSWs, a blind rotation by m more, a
sample extraction, every external product the oracle's integer one.  The device computes the same integers,
so every comparison here is word for word; there is no tolerance anywhere.  GGSWs are near-noiseless
(sigma 2^-52, as tests/test_gpu_extract_bits.py); the bit-exact checks do not depend on the noise, the decrypt
check keeps every phase inside its window.  Outputs are sentinel-filled before each call.  References are
computed once per (shape, geometry) and shared.  Besides the small shapes, the optimizer's WoP table runs at its
own ring, k = 2, N = 1024, with each of its 20 GGSW decompositions (tests/table_shapes.py).

One bound is not taken through the ABI: concrete_hip_generic_error_bound answers -1 for a (k, N, level) whose
primary key format is a hand-tuned kernel's (tests/test_keygen_abi.py asserts that), which (1, 1024, 3) and
(1, 2048, 2) are.  The residual test calls it where it answers and, for every shape, vp_reference.error_bound:
the same function on the oracle's restatement (tests/test_oracle.py holds the two together).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_shapes as S  # noqa: E402
import vp_reference as V  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY_STD = 2.0 ** -52
SENTINEL = 0x5A5A5A5A5A5A5A5A

# (k, N, level, base_log): one transform size each, both level orders, k > 1, and T = 2 sub-digits (base_log 15
# on the 13-bit limbs of (1, 1024, 2))
SHAPES = {"n512": (1, 512, 2, 10), "n1024": (1, 1024, 3, 8), "n2048": (1, 2048, 2, 12), "k2n512": (2, 512, 2, 10),
          "n1024t2": (1, 1024, 2, 15)}
# the WoP table's own ring (k = 2, N = 1024) at each of its 20 GGSW decompositions (cb_l, cb_b), up to 32 levels
WOP_SHAPES = {"wop_l%db%d" % d: S.WOP_RING + d for d in S.WOP_CB}
# one of them per general key format the CMUX kernel runs them on (tests/test_keygen_abi.py::
# test_wop_ggsw_key_formats): (limbs, bits) = (5,13) with two sub-digits, (6,12), (5,14), (4,16), (4,19), (4,20), (4,21)
WOP_FORMAT_SHAPES = ["wop_l%db%d" % d for d in [(1, 14), (4, 6), (5, 5), (6, 5), (10, 3), (16, 2), (32, 1)]]


def _geoms(N):
    """(r, m, tau, lookups)"""
    return [(0, 0, 1, 1), (0, N.bit_length() - 1, 2, 1), (1, 0, 1, 1), (3, 0, 3, 1), (3, 4, 3, 3), (2, 1, 1, 2)]


# the full geometry list at (1, 1024, 3, 8); (3, 4, 3, 3) and one more at the other shapes
CASES = [("n1024", g) for g in _geoms(1024)] + [
    ("n512", (3, 4, 3, 3)), ("n512", (0, 9, 2, 1)),
    ("n2048", (3, 4, 3, 3)), ("n2048", (2, 1, 1, 2)),
    ("k2n512", (3, 4, 3, 3)), ("k2n512", (0, 9, 2, 1)),
    ("n1024t2", (3, 4, 3, 3)), ("n1024t2", (3, 0, 3, 1))] + [(name, (3, 4, 3, 3)) for name in WOP_SHAPES]


def _case_id(c):
    return f"{c[0]}-r{c[1][0]}m{c[1][1]}t{c[1][2]}x{c[1][3]}"


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from concrete_amd import _native
    from concrete_amd import backend as B
    from oracle import pyoracle as O
    O.lib()
    return dict(torch=torch, L=_native.lib(), B=B, O=O, N=_native, keys={}, cases={})


def _params(env, shape):
    k, N, level, base_log = SHAPES[shape] if shape in SHAPES else WOP_SHAPES[shape]
    return env["B"].PbsParams(n=1, k=k, N=N, level=level, base_log=base_log)


def _index(shape):
    """A shape's number in the seeds: SHAPES sorted by name, then WOP_SHAPES in the table's order."""
    return sorted(SHAPES).index(shape) if shape in SHAPES else len(SHAPES) + list(WOP_SHAPES).index(shape)


def _key(env, shape):
    """The GLWE secret key of a shape, generated once per module."""
    if shape not in env["keys"]:
        p = _params(env, shape)
        env["keys"][shape] = env["O"].binary_key(p.k * p.N, 8100 + _index(shape))
    return env["keys"][shape]


def _patterns(rng, bits, lookups):
    """Distinct GGSW bit patterns, one per lookup, neither all 0 nor all 1 (a single bit: 1, the odd leaf)."""
    if bits == 0:
        return np.zeros((lookups, 0), dtype=np.int64)
    if bits == 1:
        assert lookups == 1
        return np.ones((1, 1), dtype=np.int64)
    vals = rng.choice(np.arange(1, (1 << bits) - 1), size=lookups, replace=False)
    return np.array([[(int(v) >> (bits - 1 - i)) & 1 for i in range(bits)] for v in vals], dtype=np.int64)


def _case(env, shape, geom, messages=False):
    """Inputs and the CPU reference of one (shape, geometry), computed once and never modified.  messages:
    the LUT coefficients are 4-bit messages in the top bits (the decrypt test) instead of random words."""
    key = (shape, geom, messages)
    if key in env["cases"]:
        return env["cases"][key]
    p = _params(env, shape)
    r, m, tau, lookups = geom
    rng = np.random.RandomState(8200 + 31 * _index(shape) + 7 * r + 3 * m + tau + 101 * lookups)
    bits = _patterns(rng, r + m, lookups)
    ggsws = V.ggsw_encrypt(_key(env, shape), bits, p.k, p.N, p.level, p.base_log, KEY_STD, 8300 + 13 * r + m)
    if messages:
        table = rng.randint(0, 16, size=(tau, 1 << r, p.N)).astype(np.uint64)
        luts = table << np.uint64(60)
    else:
        table = None
        luts = rng.randint(0, 1 << 32, size=(tau, 1 << r, p.N)).astype(np.uint64) << np.uint64(32) | \
            rng.randint(0, 1 << 32, size=(tau, 1 << r, p.N)).astype(np.uint64)
    c = dict(p=p, bits=bits, ggsws=ggsws, luts=luts, table=table)
    if not messages:
        c["lwe"], c["tree"] = V.vertical_packing(ggsws, luts, r, m, p.k, p.N, p.level, p.base_log)
        for a in (c["lwe"], c["tree"], ggsws, luts):
            a.setflags(write=False)
    if shape in SHAPES or shape in WOP_FORMAT_SHAPES:  # the other WoP shapes have one test each
        env["cases"][key] = c
    return c


def _filled(env, shape):
    t = env["torch"].empty(shape, dtype=env["torch"].int64, device=DEV)
    t.fill_(SENTINEL)  # below 2^63: the same bits as int64
    return t


def _run(env, c, geom, scratch=None, resid=None):
    B, p = env["B"], c["p"]
    r, m, tau, lookups = geom
    out = _filled(env, (lookups, tau, p.lwe_out_size))
    tree = _filled(env, (lookups, tau, p.glwe_size))
    d_ggsw = B.to_device(c["ggsws"].reshape(-1).copy(), DEV) if r + m else None  # (the cached arrays are read-only)
    lwe, tree, max_g = B.vertical_packing(p, d_ggsw, B.to_device(c["luts"].copy(), DEV), r, m, lookups, out=out,
                                          tree_out=tree, scratch=scratch, resid=resid)
    env["torch"].cuda.synchronize()
    return B.to_host(lwe), B.to_host(tree), max_g


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_bit_exact_against_the_reference(env, case):
    shape, geom = case
    c = _case(env, shape, geom)
    p = c["p"]
    assert env["B"].vertical_packing_supported(p)
    scratch = None
    if geom == (3, 4, 3, 3):  # the caller's scratch, exactly the size the query names; elsewhere the pool's
        need = env["B"].vertical_packing_scratch_bytes(p, *geom)
        assert need % 16 == 0
        scratch = env["torch"].empty(need // 8, dtype=env["torch"].int64, device=DEV)
    lwe, tree, _ = _run(env, c, geom, scratch=scratch)
    assert np.array_equal(tree, c["tree"]), "the CMUX tree's result differs from the reference"
    assert np.array_equal(lwe, c["lwe"]), "the extracted LWEs differ from the reference"


@pytest.mark.parametrize("shape", sorted(SHAPES) + WOP_FORMAT_SHAPES)
def test_residual_and_measured_spectrum(env, shape):
    """The largest rounding residual of the call stays under the certified bound evaluated at the measured
    max|G| of the call's own GGSWs, and that max|G| is what the general key conversion records for them."""
    L, B, torch = env["L"], env["B"], env["torch"]
    geom = (3, 4, 3, 3)
    c = _case(env, shape, geom)
    p = c["p"]
    resid = torch.zeros(1, dtype=torch.int64, device=DEV)
    lwe, _, max_g = _run(env, c, geom, resid=resid)
    assert np.array_equal(lwe, c["lwe"])
    seen = float(B.to_host(resid).view(np.float64)[0])
    bound = V.error_bound(p.k, p.N, p.level, p.base_log, max_g)
    abi = L.concrete_hip_generic_error_bound(p.k, p.N, p.level, p.base_log, max_g)
    print(f"{shape}: residual {seen:.3e}, bound {bound:.3e} (ABI {abi:.3e}), max|G| {max_g:.6e}")
    if abi >= 0.0:  # answers only where the primary key format is the general one (module docstring)
        assert abs(abi - bound) <= 1e-12 * bound
        assert seen <= abi
    assert 0.0 < seen <= bound < 0.5
    n = c["ggsws"].shape[0] * c["ggsws"].shape[1]
    dest = torch.empty(L.concrete_hip_generic_bsk_size_bytes(n, p.k, p.level, p.N) // 8, dtype=torch.int64, device=DEV)
    src = np.ascontiguousarray(c["ggsws"]).reshape(-1)
    env["N"].check(L.concrete_hip_convert_bsk_generic(B._stream(DEV), 0, dest.data_ptr(), src.ctypes.data, 0, n, p.k,
                                                      p.level, p.N), "concrete_hip_convert_bsk_generic")
    recorded = L.concrete_hip_key_spectrum_max(dest.data_ptr())
    assert recorded > 0 and abs(recorded - max_g) <= 1e-9 * recorded


def test_two_calls_under_the_reference_names_equal_the_fused_call(env):
    """cuda_cmux_tree_64 into cuda_blind_rotate_and_sample_extraction_64: the tree call's output is the
    rotation call's lut_vector.  One with a buffer from its scratch call, one with NULL (pool scratch)."""
    L, B, torch = env["L"], env["B"], env["torch"]
    shape, geom = "n1024", (3, 4, 3, 3)
    c = _case(env, shape, geom)
    p = c["p"]
    r, m, tau, _ = geom
    words = V.ggsw_words(p.k, p.N, p.level)
    d_ggsw = B.to_device(c["ggsws"][0].reshape(-1).copy(), DEV)  # lookup 0
    d_luts = B.to_device(c["luts"].copy(), DEV)
    glwe = _filled(env, (tau, p.glwe_size))
    lwe = _filled(env, (tau, p.lwe_out_size))
    stream = B._stream(DEV)
    buf = C.c_void_p(None)
    L.scratch_cuda_cmux_tree_64(stream, 0, C.byref(buf), p.k, p.N, p.level, r, tau, 0, True)
    assert buf.value
    L.cuda_cmux_tree_64(stream, 0, glwe.data_ptr(), d_ggsw.data_ptr(), d_luts.data_ptr(), buf, p.k, p.N, p.base_log,
                        p.level, r, tau, 0)
    L.cleanup_cuda_cmux_tree(stream, 0, C.byref(buf))
    assert not buf.value
    L.scratch_cuda_blind_rotation_sample_extraction_64(stream, 0, C.byref(buf), p.k, p.N, p.level, m, tau, 0, False)
    assert not buf.value
    L.cuda_blind_rotate_and_sample_extraction_64(stream, 0, lwe.data_ptr(), d_ggsw.data_ptr() + 8 * r * words,
                                                 glwe.data_ptr(), None, m, tau, p.k, p.N, p.base_log, p.level, 0)
    L.cleanup_cuda_blind_rotation_sample_extraction(stream, 0, C.byref(buf))
    fused_lwe, fused_tree, _ = B.vertical_packing(p, d_ggsw, d_luts, r, m, 1, want_tree=True)
    torch.cuda.synchronize()
    assert np.array_equal(B.to_host(glwe), B.to_host(fused_tree)[0])
    assert np.array_equal(B.to_host(lwe), B.to_host(fused_lwe)[0])
    assert np.array_equal(B.to_host(lwe), c["lwe"][0])


@pytest.mark.parametrize("shape,m", [("n1024", 8), ("n1024", 10), ("n2048", 8), ("n2048", 11)])
def test_rotation_equals_the_pbs_kernels(env, shape, m):
    """r = 0: the rotation alone is a PBS of n = m on the synthetic LWE rows of vp_reference, with the rotation
    GGSWs (in application order) as the bootstrapping key: the PBS kernels this backend already has must give
    the same words."""
    B, torch = env["B"], env["torch"]
    p = _params(env, shape)
    tau = 2
    rng = np.random.RandomState(8400 + m)
    bits = _patterns(rng, m, 1)
    ggsws = V.ggsw_encrypt(_key(env, shape), bits, p.k, p.N, p.level, p.base_log, KEY_STD, 8500 + m)
    luts = rng.randint(0, 1 << 32, size=(tau, 1, p.N)).astype(np.uint64) << np.uint64(32) | \
        rng.randint(0, 1 << 32, size=(tau, 1, p.N)).astype(np.uint64)
    out = _filled(env, (1, tau, p.lwe_out_size))
    got, _, _ = B.vertical_packing(p, B.to_device(ggsws.reshape(-1), DEV), B.to_device(luts, DEV), 0, m, 1, out=out)
    pp = B.PbsParams(n=m, k=p.k, N=p.N, level=p.level, base_log=p.base_log)
    fbsk = B.convert_bsk(pp, V.pbs_key(ggsws[0]), DEV)
    accs = np.stack([B.trivial_glwe(pp, luts[o, 0]) for o in range(tau)])
    rows = np.tile(V.synthetic_lwe(m, p.N), (tau, 1))
    want = B.pbs(pp, fbsk, B.to_device(rows, DEV), B.to_device(accs, DEV),
                 lut_idx=B.to_device(np.arange(tau, dtype=np.uint64), DEV))
    torch.cuda.synchronize()
    assert np.array_equal(B.to_host(got)[0], B.to_host(want))


def _const_ggsw_spectrum(k, N, level):
    """max|G| of a GGSW whose every word is 0x5555...: the limb spectra of the constant polynomial, in f64."""
    from oracle import keyref
    bits = V.limb_bits(k, N, level)
    limbs = keyref.limbs_generic(np.full(N, 0x5555555555555555, dtype=np.uint64), bits, -(-64 // bits))
    M = N // 2
    zeta = np.exp(1j * np.pi * np.arange(M) / N)
    return max(float(np.abs(np.fft.fft((lim[:M].astype(np.float64) + 1j * lim[M:].astype(np.float64)) * zeta)).max())
               for lim in limbs)


def test_gate_refuses_ggsws_with_a_large_spectrum(env):
    """GGSWs whose every word is 0x5555...: base_log is picked on the CPU as the smallest for which the bound at
    their max|G| reaches 1/2 while the static gate (generic_pbs_ok) still accepts it, at level 3 or, if none
    exists there, level 1.  At k = 1, N = 2048 (at N = 512 and 1024 no level has such a base_log: the constant
    GGSW's spectrum is only 1.7x the random-key estimate there) level 3 has none and level 1 has base_log 40,
    which is what this test runs: four sub-digits on the 13-bit limbs.  The call returns -2 and writes nothing;
    at base_log 7 the same GGSWs run and are bit-exact."""
    L, B, torch = env["L"], env["B"], env["torch"]
    k, N = 1, 2048
    pick = None
    for level in (3, 1):
        g = _const_ggsw_spectrum(k, N, level)
        for b in range(1, 64 // level + 1):
            if V.generic_pbs_ok(k, N, level, b) and V.error_bound(k, N, level, b, g) >= 0.5:
                pick = (level, b, g)
                break
        if pick:
            break
    assert pick is not None, "no base_log passes the static gate and fails the measured one"
    level, base_log, g = pick
    print(f"gate test: level {level}, base_log {base_log}, max|G| {g:.6e}, "
          f"bound {V.error_bound(k, N, level, base_log, g):.4f}")
    assert (level, base_log) == (1, 40)
    r, m, tau = 1, 1, 1
    ggsws = np.full((1, r + m, level, k + 1, k + 1, N), 0x5555555555555555, dtype=np.uint64)
    rng = np.random.RandomState(8600)
    luts = rng.randint(0, 1 << 32, size=(tau, 1 << r, N)).astype(np.uint64) << np.uint64(32) | \
        rng.randint(0, 1 << 32, size=(tau, 1 << r, N)).astype(np.uint64)
    d_ggsw, d_luts = B.to_device(ggsws.reshape(-1), DEV), B.to_device(luts, DEV)
    bad = B.PbsParams(n=1, k=k, N=N, level=level, base_log=base_log)
    assert B.vertical_packing_supported(bad)
    out = _filled(env, (1, tau, bad.lwe_out_size))
    tree = _filled(env, (1, tau, bad.glwe_size))
    max_g = C.c_double(-1.0)
    rc = L.concrete_hip_vertical_packing(B._stream(DEV), 0, out.data_ptr(), tree.data_ptr(), d_ggsw.data_ptr(),
                                         d_luts.data_ptr(), k, N, base_log, level, r, m, tau, 1, None, 0, None,
                                         C.byref(max_g))
    torch.cuda.synchronize()
    assert rc == -2, L.concrete_hip_last_error()
    assert abs(max_g.value - g) <= 1e-9 * g  # the refusal reports the spectrum that caused it
    sentinel = np.uint64(SENTINEL)
    assert (B.to_host(out) == sentinel).all() and (B.to_host(tree) == sentinel).all()
    good = B.PbsParams(n=1, k=k, N=N, level=level, base_log=7)
    out = _filled(env, (1, tau, good.lwe_out_size))
    tree = _filled(env, (1, tau, good.glwe_size))
    lwe, tree, measured = B.vertical_packing(good, d_ggsw, d_luts, r, m, 1, out=out, tree_out=tree)
    torch.cuda.synchronize()
    assert abs(measured - g) <= 1e-9 * g
    want_lwe, want_tree = V.vertical_packing(ggsws, luts, r, m, k, N, level, 7)
    assert np.array_equal(B.to_host(tree), want_tree)
    assert np.array_equal(B.to_host(lwe), want_lwe)


def test_every_lookup_decrypts_to_the_entry_its_bits_select(env):
    B, O = env["B"], env["O"]
    shape, geom = "n1024", (3, 4, 3, 3)
    c = _case(env, shape, geom, messages=True)
    p = c["p"]
    r, m, tau, lookups = geom
    # worst-case drift of r + m CMUXes against half the 2^60 window of a 4-bit message (vp_reference's budget)
    assert (r + m) * (p.k * p.N + 1) * 2 ** (63 - p.level * p.base_log) < 2 ** 59
    lwe, _, _ = _run(env, c, geom)
    for lk in range(lookups):
        pi, ci = V.selected(c["luts"], c["bits"][lk, :r], c["bits"][lk, r:])
        dec = O.lwe_decrypt_batch(_key(env, shape), np.ascontiguousarray(lwe[lk]), p.k * p.N)
        got = [((int(d) + (1 << 59)) >> 60) % 16 for d in dec]
        assert got == [int(c["table"][o, pi, ci]) for o in range(tau)], f"lookup {lk}"
