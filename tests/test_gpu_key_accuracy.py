"""Every device Fourier key format against the long-double reference of oracle/keyref.py, every
stored element.

The certified rounding bounds rest on the accuracy of the converted key: the hand-tuned formats
(bsk.hip, double-double transform) charge only u |G| for it — a correctly rounded spectrum — and the
general format (pbs_generic.hip, plain f64 transform) charges ||dG||_2 <= gamma ||g||_2.  The PBS
tests cannot see either premise fail: a conversion of f64 accuracy would still give bit-exact
products on random keys.  Here the key itself is compared, at the smallest shape of every layout
and code path, on keys of uniform random words with planted polynomials (a constant one, all-ones
words, single coefficients at j = M and j = N - 1) in the corner positions of the layout.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import keyref as K

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
CRAFTED = 0x5555555555555555  # as tests/test_gpu_robustness.py: limb spectra ~8x a random key's
ONES = 0xFFFFFFFFFFFFFFFF

# Cap on the share of components of a double-double format that are not bit-identical to the rounded
# reference: four times the share by which two correct long-double transforms differ (K.LD_SHARE,
# measured and asserted on the CPU in tests/test_keyref.py; the device's double-double arithmetic and
# the reference are different algorithms of like precision, hence the factor), which must stay at
# most a tenth of the share by which an f64 transform differs (K.F64_SHARE), so that a conversion
# that silently dropped to f64 accuracy is ten times over the cap.
SHARE_CAP = 4.0 * K.LD_SHARE
assert SHARE_CAP <= K.F64_SHARE / 10.0

# (k, N, l), each the smallest shape that reaches its layout or code path.  GENERIC_SHAPES: the
# general-format key of that shape through concrete_hip_convert_bsk_generic (the companion of a
# hand-tuned shape, else the shape's own format)
DD_SHAPES = [
    (1, 1024, 1), (1, 1024, 2), (1, 1024, 3),                      # N1024: 3 limbs of 22/21/21 bits
    (1, 2048, 1), (1, 2048, 2), (1, 2048, 4),                      # N2048: K+-, 4 limbs
    (2, 1024, 1), (2, 1024, 2), (2, 1024, 3),                      # K2N1024: 3 = the first level-major one
    (3, 512, 1), (3, 512, 3), (4, 512, 1), (4, 512, 2), (4, 512, 3), (5, 256, 1), (6, 256, 1),  # SMALL
]
GENERIC_SHAPES = [
    (1, 1024, 1), (2, 512, 2), (2, 256, 5),    # natural order: a companion; k > 1, l > 1 (13 and 16 bit limbs)
    (1, 2048, 1), (1, 4096, 1), (1, 16384, 2),  # four-step order: a companion, one row, two levels
    (1, 32768, 1), (1, 65536, 1),               # split conversion (n = 1)
]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from concrete_amd import _native
    from concrete_amd import backend as B
    return dict(torch=torch, L=_native.lib(), B=B)


def _corners(n, k, l):
    """Four distinct corner polynomials (i, level v, row, col) of the standard layout
    [n][l][row][col]: the first; the last i / level / row / column; the last row at the far end of
    the level order; the last column of the last i."""
    k1 = k + 1
    at = lambda i, v, r, c: ((i * l + v) * k1 + r) * k1 + c
    out = [at(0, 0, 0, 0), at(n - 1, l - 1, k, k), at(0, l - 1, k, 0), at(n - 1, 0, 0, k)]
    assert len(set(out)) == 4
    return out


def _planted_key(n, k, N, l, seed):
    """Uniform random u64 words (the limbs span their full range; the key need not be an
    encryption) with the planted polynomials at the corners; the constant CRAFTED one first."""
    rng = np.random.RandomState(seed)
    npoly = n * l * (k + 1) ** 2
    w = rng.randint(0, 2 ** 32, size=(npoly, N, 2), dtype=np.int64).astype(np.uint64)
    key = (w[..., 0] << np.uint64(32)) | w[..., 1]
    a, b, c, d = _corners(n, k, l)
    key[a] = CRAFTED
    key[b] = ONES
    key[c] = 0
    key[c, N // 2] = 0x7FFFFFFFFFFFFFFF
    key[d] = 0
    key[d, N - 1] = 0x8000000000000000
    return key, (a, b, c, d)


def _convert(env, n, k, N, l, words, general, device_source=False):
    """The device key (the tensor that holds it), from a host source or (device_source) a copy of it on
    the device, read in place with src_is_device = 1.  The conversion refuses (-2)
    a key whose recorded max|G| leaves no base_log with a certified bound below 1/2 — the planted
    constant polynomial does that to some formats — after storing and recording it: the refusal
    must be exactly that, and the stored key is compared all the same."""
    torch, L, B = env["torch"], env["L"], env["B"]
    p = B.PbsParams(n=n, k=k, N=N, level=l, base_log=1, ks_level=1, ks_base_log=1)
    nbytes = L.concrete_hip_generic_bsk_size_bytes(n, k, l, N) if general else B.fourier_bsk_bytes(p)
    assert nbytes > 0
    out = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda:0")
    src = np.ascontiguousarray(words.reshape(-1), dtype=np.uint64)
    assert src.size == p.bsk_len
    s = torch.cuda.current_stream().cuda_stream
    fn = L.concrete_hip_convert_bsk_generic if general else L.concrete_hip_convert_bsk
    d_src = B.to_device(src, "cuda:0") if device_source else None
    rc = fn(s, 0, out.data_ptr(), d_src.data_ptr() if device_source else src.ctypes.data, int(device_source), n, k, l,
            N)
    torch.cuda.synchronize()
    assert rc in (0, -2), rc
    assert (rc == -2) == (not L.concrete_hip_key_error_bound(out.data_ptr(), 1) < 0.5)
    return out


def _format(env, n, k, N, l, general):
    B = env["B"]
    kind, limbs, bits = B.bsk_format(B.PbsParams(n=n, k=k, N=N, level=l, base_log=1))
    if general:
        gbits = K.generic_limb_bits(k, N, l)
        glimbs = -(-64 // gbits)
        if kind == K.KIND_GENERIC:
            assert (limbs, bits) == (glimbs, gbits)
        assert env["L"].concrete_hip_generic_bsk_size_bytes(n, k, l, N) == n * (k + 1) ** 2 * l * glimbs * (N // 2) * 16
        return K.KIND_GENERIC, glimbs, gbits
    assert kind not in (0, K.KIND_GENERIC), "the table's level is not one this hand-tuned format accepts"
    return kind, limbs, bits


def _check_recorded_max(env, n, k, N, l, general, key, planted, ref, fk):
    """concrete_hip_key_spectrum_max == the reference's max|G| over the whole key to 1e-12, with the
    constant polynomial at each corner in turn (swapped with the polynomial that was there: the set
    of spectra, and so the expected maximum, stays; no block, limb or tail element escapes
    spec_max_commit).  The reference's argmax is the planted polynomial."""
    L = env["L"]
    want = ref.max_spectrum
    assert ref.argmax_poly_limb[0] == planted[0]
    assert abs(L.concrete_hip_key_spectrum_max(fk.data_ptr()) / want - 1.0) <= 1e-12
    for pos in planted[1:]:
        moved = key.copy()
        moved[[planted[0], pos]] = moved[[pos, planted[0]]]
        fk2 = _convert(env, n, k, N, l, moved, general)
        got = L.concrete_hip_key_spectrum_max(fk2.data_ptr())
        assert abs(got / want - 1.0) <= 1e-12, (pos, got, want)


@pytest.mark.parametrize("shape", DD_SHAPES, ids=lambda s: "k%d-N%d-l%d" % s)
def test_double_double_key_is_correctly_rounded(env, shape):
    """Hand-tuned formats (all of bsk.hip; for N2048 the stored K+ and K-, formed in long double
    from G_e, G_o and s_f).  With ref the long-double value with the stored scale applied:

    1. certificate, every component: |dev - ref| <= u |ref| + 2 ld_allowance(||z||_2, M) scale
       (correct rounding; the reference's and the device's 2^-64-precise twiddle tables), where at
       M <= 512 the second term is itself at most 2 u rms of the block's components;
    2. not silently f64: the share of the random polynomials' components with dev != float64(ref)
       is at most SHARE_CAP = 4 x 0.7 % = 2.8 % (two long-double transforms differ in 0.56 .. 0.63 %,
       numpy's f64 FFT in 75.7 .. 78.0 %: tests/test_keyref.py), and every differing component is
       within 1 ulp or within the allowance of 1;
    3. the recorded max|G| (_check_recorded_max).
    Measured on an MI355X: shares 0.28 .. 0.35 % over the 16 shapes."""
    k, N, l = shape
    n = 2
    kind, limbs, bits = _format(env, n, k, N, l, False)
    key, planted = _planted_key(n, k, N, l, 9100 + 7 * N + 31 * k + l)
    fk = _convert(env, n, k, N, l, key, False)
    dev = env["B"].to_host(fk).view(np.float64).reshape(-1, 2)
    ref = K.reference_key(kind, key, n, k, N, l, limbs, bits)
    m = ref.map
    assert dev.shape[0] == ref.re.size

    allow = 2.0 * K.ld_allowance(ref.znorm, m.m_eff) * m.scale
    if m.m_eff <= 512:
        assert np.all(allow <= 2.0 * U * ref.znorm * m.scale / np.sqrt(2.0))
    random_poly = ~np.isin(m.poly, planted)
    differ = 0
    for c, r in ((0, ref.re), (1, ref.im)):
        d = dev[:, c]
        err = np.abs(d.astype(LD) - r).astype(np.float64)
        bound = U * np.abs(r).astype(np.float64) + allow
        bad = np.flatnonzero(~(err <= bound))
        assert bad.size == 0, (shape, c, bad[:4], err[bad[:4]], bound[bad[:4]])
        r64 = r.astype(np.float64)
        ne = d != r64
        assert np.all((np.abs(d - r64)[ne] <= np.spacing(np.abs(r64[ne]))) | (err[ne] <= allow[ne]))
        differ += int(np.count_nonzero(ne & random_poly))
    share = differ / (2.0 * np.count_nonzero(random_poly))
    print(f"key accuracy k={k} N={N} l={l} kind={kind}: share of components != rounded reference {share:.4%}")
    assert share <= SHARE_CAP, (shape, share)
    _check_recorded_max(env, n, k, N, l, False, key, planted, ref, fk)


@pytest.mark.parametrize("shape", GENERIC_SHAPES, ids=lambda s: "k%d-N%d-l%d" % s)
def test_general_key_is_within_its_charged_error(env, shape):
    """General format (gen_convert_kernel: natural order below N = 2048, four-step order to 16384;
    the split conversion at 32768 / 65536), every block (i, col, limb, row, q):

        || dev M - ref ||_2  <=  gamma_gen sqrt(M) ||z||_2 + ld_allowance(||z||_2, M)

    with gamma_gen exactly as pyoracle.generic_error_bound (mu = 5u, 2 log2 M stages).  Norm
    convention: generic_error_bound charges ||dG||_2 <= gamma ||g||_2 for the unitary transform
    G / sqrt(M) of the folded, twisted limb polynomial z, ||z||_2 = ||g||_2 (the twist has modulus 1);
    the key stores G / M, so dev M - ref is the error of the unnormalised spectrum, sqrt(M) times
    the unitary one.  ||z||_2 is the actual norm of that limb polynomial (generic_error_bound uses
    its worst case gnorm = sqrt(N) 2^(b-1)).  The largest ratio err / (gamma_gen sqrt(M) ||z||_2) is
    printed; measured on an MI355X it is 0.0064 .. 0.0133 over N = 256 .. 65536.  Then the
    recorded
    max|G| (_check_recorded_max)."""
    k, N, l = shape
    n = 1 if N >= 32768 else 2
    M = N // 2
    kind, limbs, bits = _format(env, n, k, N, l, True)
    key, planted = _planted_key(n, k, N, l, 9300 + 7 * (N % 1009) + 31 * k + l)
    fk = _convert(env, n, k, N, l, key, True)
    dev = env["B"].to_host(fk).view(np.float64).reshape(-1, M, 2)
    ref = K.reference_key(kind, key, n, k, N, l, limbs, bits)
    assert dev.shape[0] * M == ref.re.size and ref.map.scale == 1.0 / M
    dre = (dev[..., 0].astype(LD) - ref.re.reshape(-1, M)) * LD(M)
    dim = (dev[..., 1].astype(LD) - ref.im.reshape(-1, M)) * LD(M)
    err = np.sqrt(np.sum(dre * dre + dim * dim, axis=1)).astype(np.float64)
    zn = ref.znorm.reshape(-1, M)
    assert np.all(zn == zn[:, :1])  # a block is one limb polynomial
    zn = zn[:, 0]
    charged = K.gamma_generic(M) * np.sqrt(M) * zn
    bound = charged + K.ld_allowance(zn, M)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (shape, bad[:4], err[bad[:4]], bound[bad[:4]])
    ratio = float(np.max(err[zn > 0] / charged[zn > 0]))
    print(f"key accuracy general k={k} N={N} l={l} bits={bits}: max err / (gamma sqrt(M) ||z||) = {ratio:.4f}")
    _check_recorded_max(env, n, k, N, l, True, key, planted, ref, fk)


def test_general_shapes_cover_both_limb_kinds():
    """The general-format shapes include a limb width that divides 64 and one that does not (the top
    limb is then narrower than the others)."""
    bits = [K.generic_limb_bits(k, N, l) for k, N, l in GENERIC_SHAPES]
    assert any(64 % b == 0 for b in bits) and any(64 % b != 0 for b in bits), bits


@pytest.mark.parametrize("general", [False, True], ids=["own-format", "general-format"])
@pytest.mark.parametrize("shape", [(1, 1024, 1), (1, 2048, 1)], ids=lambda s: "k%d-N%d-l%d" % s)
def test_host_and_device_sources_give_the_same_key(env, shape, general):
    """Both convert entry points stage a host source and read a device source in place: the stored keys are
    equal in every byte, and so is the recorded max|G|."""
    k, N, l = shape
    n = 2
    key, _ = _planted_key(n, k, N, l, 9500 + 7 * N + l)
    L, B = env["L"], env["B"]
    got = []
    for device_source in (False, True):
        fk = _convert(env, n, k, N, l, key, general, device_source)
        got.append((B.to_host(fk).copy(), L.concrete_hip_key_spectrum_max(fk.data_ptr())))
    assert got[0][1] > 0.0 and got[0][1] == got[1][1]
    assert np.array_equal(got[0][0], got[1][0])


def _scratch_round_trip(env, scratch, cleanup, use):
    """scratch(buf, allocate) and cleanup(buf) of one family; use(buf) is the family's own call."""
    L, torch = env["L"], env["torch"]
    buf = C.c_void_p(None)
    scratch(C.byref(buf), False)
    assert not buf.value  # allocate_gpu_memory = false: NULL, the call takes pool scratch
    cleanup(C.byref(buf))  # a no-op on NULL
    scratch(C.byref(buf), True)
    assert buf.value
    use(buf)  # accepted between scratch and cleanup (a buffer that is refused aborts the process)
    torch.cuda.synchronize()
    cleanup(C.byref(buf))
    assert not buf.value
    cleanup(C.byref(buf))  # a second cleanup is a no-op
    assert not buf.value
    assert L.concrete_hip_device_status(0) == 0


def test_scratch_round_trip_of_both_families(env):
    """scratch_cuda_* / cleanup_cuda_* of bit extraction and of vertical packing (its two calls), each at
    the smallest shape its call supports, on all-zero keys and inputs (a zero key passes every gate; the
    results are checked in tests/test_gpu_extract_bits.py and tests/test_gpu_vertical_packing.py)."""
    L, torch = env["L"], env["torch"]
    s = torch.cuda.current_stream().cuda_stream
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda:0")

    # bit extraction: the PBS shape of test_rotation_equals_the_pbs_kernels (k = 1, N = 1024, l = 3, n = 8),
    # a one-level keyswitch; one row of 2 bits (keyswitch, PBS, keyswitch)
    k, N, l, logb, n, ksl, ksb, nb, dl = 1, 1024, 3, 8, 8, 1, 1, 2, 62
    assert L.concrete_hip_extract_bits_supported(k * N, n, k, N, logb, l, ksb, ksl) == 1
    fk = _convert(env, n, k, N, l, np.zeros(n * l * (k + 1) ** 2 * N, dtype=np.uint64), False)
    ksk, inp, out = zeros(ksl * k * N * (n + 1)), zeros(k * N + 1), zeros(nb * (n + 1))
    _scratch_round_trip(
        env, lambda b, alloc: L.scratch_cuda_extract_bits_64(s, 0, b, k, n, N, l, 1, 0, alloc),
        lambda b: L.cleanup_cuda_extract_bits(s, 0, b),
        lambda b: L.cuda_extract_bits_64(s, 0, out.data_ptr(), inp.data_ptr(), b, ksk.data_ptr(), fk.data_ptr(), nb, dl,
                                         k * N, n, k, N, logb, l, ksb, ksl, 1, 0))

    # vertical packing: k = 1, N = 512 (tests/test_gpu_vertical_packing.py SHAPES); one tree layer, one rotation
    k, N, l, logb, tau = 1, 512, 2, 10, 1
    assert L.concrete_hip_vertical_packing_supported(k, N, l, logb) == 1
    ggsw, luts, glwe, lwe = zeros(l * (k + 1) ** 2 * N), zeros(tau * 2 * N), zeros(tau * (k + 1) * N), zeros(k * N + 1)
    _scratch_round_trip(
        env, lambda b, alloc: L.scratch_cuda_cmux_tree_64(s, 0, b, k, N, l, 1, tau, 0, alloc),
        lambda b: L.cleanup_cuda_cmux_tree(s, 0, b),
        lambda b: L.cuda_cmux_tree_64(s, 0, glwe.data_ptr(), ggsw.data_ptr(), luts.data_ptr(), b, k, N, logb, l, 1, tau,
                                      0))
    _scratch_round_trip(
        env, lambda b, alloc: L.scratch_cuda_blind_rotation_sample_extraction_64(s, 0, b, k, N, l, 1, tau, 0, alloc),
        lambda b: L.cleanup_cuda_blind_rotation_sample_extraction(s, 0, b),
        lambda b: L.cuda_blind_rotate_and_sample_extraction_64(s, 0, lwe.data_ptr(), ggsw.data_ptr(), glwe.data_ptr(),
                                                               b, 1, tau, k, N, logb, l, 0))
