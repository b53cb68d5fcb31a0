"""CPU tests of oracle/keyref.py, the long-double reference that tests/test_gpu_key_accuracy.py
compares every device Fourier key format with: the limb splits, closed forms of the folded, twisted
transform, agreement of independent extended-precision transforms (which also measures the two
shares the GPU test's cap is derived from), and the index maps of every key layout."""
import ctypes as C
from decimal import Decimal, getcontext

import numpy as np
import pytest

from oracle import keyref as K

LD = np.longdouble
M64 = (1 << 64) - 1
EPS = 2.0 ** -64
U = 2.0 ** -53

# every (L) of the equal-width split and every (bits, L) of the general format that a key format
# uses (hand-tuned: 3 x 22/21/21, 4 x 16, 5 x 13/13/13/13/12; general: concrete_hip_bsk_format over
# the shapes of test_general_formats_are_covered, which include widths that do not divide 64)
EQUAL_L = (3, 4, 5)
GENERIC_FORMATS = ((8, 8), (9, 8), (10, 7), (11, 6), (12, 6), (13, 5), (14, 5), (15, 5), (16, 4), (17, 4),
                   (19, 4), (21, 4), (22, 3), (24, 3))


def _edge_words(widths):
    """0, 1, 2^64 - 1, 2^63, 2^63 - 1, every limb at +half (stored as -half with a carry), every
    limb at half - 1, and a carry that ripples through all limbs."""
    shifts = np.concatenate(([0], np.cumsum(widths)[:-1]))
    all_half = sum(1 << (int(s) + w - 1) for s, w in zip(shifts, widths)) & M64
    all_half_m1 = sum(((1 << (w - 1)) - 1) << int(s) for s, w in zip(shifts, widths)) & M64
    # lowest limb at half, every higher limb at half - 1: the carry of each limb makes the next one half
    ripple = ((1 << (widths[0] - 1)) + sum(((1 << (w - 1)) - 1) << int(s) for s, w in zip(shifts[1:], widths[1:]))) & M64
    return [0, 1, M64, 1 << 63, (1 << 63) - 1, all_half, all_half_m1, ripple]


def _check_split(limbs, words, widths):
    shifts = np.concatenate(([0], np.cumsum(widths)[:-1]))
    for idx, w in enumerate(words):
        col = [int(limbs[t][idx]) for t in range(len(widths))]
        assert sum(v << int(s) for v, s in zip(col, shifts)) & M64 == int(w), (hex(int(w)), col)
        for v, wd in zip(col, widths):
            assert -(1 << (wd - 1)) <= v < (1 << (wd - 1)), (hex(int(w)), col, widths)


def test_limb_splits_recombine_and_stay_balanced(oracle):
    rng = np.random.RandomState(11)
    rnd = [int(a) << 32 | int(b) for a, b in rng.randint(0, 2 ** 32, size=(500, 2), dtype=np.int64)]
    for L in EQUAL_L:
        widths = K.equal_widths(L)
        assert sum(widths) == 64 and max(widths) - min(widths) <= 1 and widths == sorted(widths, reverse=True)
        words = _edge_words(widths) + rnd
        limbs = K.limbs_equal(np.array(words, dtype=np.uint64), L)
        assert limbs.dtype == np.int64 and limbs.shape == (L, len(words))
        _check_split(limbs, words, widths)
        # Python integers give the same limbs; the oracle's ora_limb_split (the C restatement) too
        buf = (C.c_int64 * L)()
        for idx, w in enumerate(words[:40]):
            assert [int(v) for v in K.limbs_equal(w, L)] == [int(limbs[t][idx]) for t in range(L)]
            oracle.lib().ora_limb_split(C.c_uint64(w), L, buf)
            assert list(buf) == [int(limbs[t][idx]) for t in range(L)], (hex(w), L)
    for bits, L in GENERIC_FORMATS:
        widths = K.generic_widths(bits, L)
        assert sum(widths) == 64 and 0 < widths[-1] <= bits
        words = _edge_words(widths) + rnd
        limbs = K.limbs_generic(np.array(words, dtype=np.uint64), bits, L)
        assert limbs.dtype == np.int64 and limbs.shape == (L, len(words))
        _check_split(limbs, words, widths)
        assert [int(v) for v in K.limbs_generic(words[7], bits, L)] == [int(limbs[t][7]) for t in range(L)]
    assert any(64 % b for b, _ in GENERIC_FORMATS) and any(64 % b == 0 for b, _ in GENERIC_FORMATS)
    # the edge words do what they are named for: all limbs at -half, and a carry through every limb
    w4 = K.equal_widths(4)
    e = K.limbs_equal(np.array(_edge_words(w4), dtype=np.uint64), 4)
    assert [int(v) for v in e[:, 5]] == [-(1 << 15), -(1 << 15) + 1, -(1 << 15) + 1, -(1 << 15) + 1]
    assert [int(v) for v in e[:, 7]] == [-(1 << 15)] * 4


def test_general_formats_are_covered():
    """GENERIC_FORMATS holds the (bits, limbs) of every general-format shape the GPU test converts
    and of the optimizer's rows; keyref.generic_limb_bits restates the library's choice (read from
    concrete_hip_bsk_format where the shape's own format is the general one; no GPU needed)."""
    from concrete_amd import _native
    from concrete_amd import backend as B
    L = _native.lib()
    for k, N, l in ((1, 1024, 1), (2, 512, 2), (2, 256, 5), (1, 2048, 1), (1, 4096, 1), (1, 16384, 2), (1, 32768, 1),
                    (1, 65536, 1), (1, 8192, 1), (1, 32768, 2), (1, 65536, 2), (3, 512, 1), (5, 256, 1), (2, 512, 1),
                    (1, 512, 4), (8, 256, 3)):
        nbytes = L.concrete_hip_generic_bsk_size_bytes(2, k, l, N)
        assert nbytes > 0
        limbs = nbytes // (2 * (k + 1) ** 2 * l * (N // 2) * 16)
        bits = K.generic_limb_bits(k, N, l)
        assert limbs == -(-64 // bits) and (bits, limbs) in GENERIC_FORMATS, (k, N, l, bits, limbs)
        kind, flimbs, fbits = B.bsk_format(B.PbsParams(n=2, k=k, N=N, level=l, base_log=1))
        if kind == K.KIND_GENERIC:
            assert (fbits, flimbs) == (bits, limbs), (k, N, l)


# ------------------------------------------------------------------------------------------
# twiddles against an independent 50-digit evaluation
# ------------------------------------------------------------------------------------------
getcontext().prec = 60
PI_DEC = Decimal("3.14159265358979323846264338327950288419716939937510582097494")


def _dec_cos_sin(x: Decimal):
    c, s, term, n = Decimal(0), Decimal(0), Decimal(1), 0
    while abs(term) > Decimal(10) ** -55:
        if n % 2 == 0:
            c += term if n % 4 == 0 else -term
        else:
            s += term if n % 4 == 1 else -term
        n += 1
        term = term * x / n
    return c, s


def _dec_to_ld(d: Decimal):
    hi = float(d)
    return LD(hi) + LD(float(d - Decimal(hi)))


def test_twiddles_are_accurate_to_64_bits():
    """exp(i pi num / den) of cis_ld against a 50-digit Taylor evaluation: within 2^-62.  A pi of 53
    bits (error 1.2e-16 = 2^-53 at the largest angle) or twiddles rounded to f64 fail this by a
    factor of several hundred."""
    worst = 0.0
    cases = [(n, 1024) for n in (1, 3, 511, 512, 513, 1023, 1024, 1025, 2047, 2049, -5, 4097)]
    cases += [(n, 65536) for n in (1, 32767, 65535, 65537, 98303, -4 * 32767 * 32765 + 32767)]
    cases += [(1 - 4 * f, 2048) for f in (0, 1, 255, 511)] + [(-2 * t, 512) for t in (1, 100, 255)]
    for num, den in cases:
        r = num % (2 * den)
        c, s = _dec_cos_sin(PI_DEC * r / den if r <= den else PI_DEC * (r - 2 * den) / den)
        got = K.cis_ld(num, den)
        worst = max(worst, abs(float(got.real - _dec_to_ld(c))), abs(float(got.imag - _dec_to_ld(s))))
    assert worst <= 2.0 ** -62, worst


# ------------------------------------------------------------------------------------------
# closed forms
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_monomial_spectra_are_pure_phases(N):
    """g = X^j: z has one non-zero entry, zeta^j at j < M and i zeta^(j-M) at j >= M (the fold), so
    G_f = exp(i pi (j - 4 j f) / N) resp. exp(i pi (N/2 + j' - 4 j' f) / N), j' = j - M; the angles
    are computed here from the reduced integers."""
    M = N // 2
    f = np.arange(M, dtype=np.int64)
    for j in (0, 1, M - 1, M, N - 1):
        g = np.zeros(N, dtype=np.int64)
        g[j] = 1
        re, im = K.spectrum_ld(g, N)
        jj = j if j < M else j - M
        want = K.cis_ld((jj - 4 * jj * f + (0 if j < M else N // 2)) % (2 * N), N)
        err = max(float(np.max(np.abs(re - want.real))), float(np.max(np.abs(im - want.imag))))
        # |G_f| = 1 and at most log2 M twiddle products touch it, each within Higham's eta: gamma, plus
        # the twist entry and the expected value's own rounding
        assert err <= K.ld_allowance(1.0, M) / np.sqrt(M) + 4 * EPS, (N, j, err)
    # the sign: -X^j is the negated spectrum exactly
    g = np.zeros(N, dtype=np.int64)
    g[N - 1] = -1
    re2, im2 = K.spectrum_ld(g, N)
    assert np.array_equal(re2, -re) and np.array_equal(im2, -im)


def test_linearity_and_parseval():
    rng = np.random.RandomState(12)
    for N in (256, 1024, 8192):
        M = N // 2
        a = rng.randint(-2 ** 21, 2 ** 21, size=N).astype(np.int64)
        b = rng.randint(-2 ** 21, 2 ** 21, size=N).astype(np.int64)
        ra, ia = K.spectrum_ld(a, N)
        rb, ib = K.spectrum_ld(b, N)
        rc, ic = K.spectrum_ld(3 * a - 5 * b, N)
        na, nb = np.sqrt(float(np.sum(a.astype(object) ** 2))), np.sqrt(float(np.sum(b.astype(object) ** 2)))
        tol = 2.0 * (K.ld_allowance(3 * na, M) + K.ld_allowance(5 * nb, M))
        assert float(np.max(np.abs(rc - (3 * ra - 5 * rb)))) <= tol
        assert float(np.max(np.abs(ic - (3 * ia - 5 * ib)))) <= tol
        # Parseval: sum |G|^2 = M sum |z|^2 = M sum g^2, the right-hand side exact in integers
        rhs = M * int(np.sum(a.astype(object) ** 2))
        lhs = np.sum(ra * ra + ia * ia)
        gamma = K.ld_allowance(1.0, M) / np.sqrt(M)
        assert abs(float(lhs / LD(rhs) - 1)) <= 2.0 * gamma + gamma * gamma + 4 * EPS


# ------------------------------------------------------------------------------------------
# two independent extended-precision transforms agree; the measured shares
# ------------------------------------------------------------------------------------------
def _direct_dft(z, M):
    j = np.arange(M, dtype=np.int64)
    W = K.cis_ld(-2 * ((j[:, None] * j[None, :]) % M), M)  # exp(-2 pi i j f / M), angle reduced mod M
    return np.stack([(W * zz[None, :]).sum(axis=1) for zz in z])


def _share(a, b):
    return float(np.mean(np.asarray(a, dtype=np.float64) != np.asarray(b, dtype=np.float64)))


def test_independent_long_double_transforms_agree(oracle):
    """spectrum_ld against (a) an O(M^2) direct long-double DFT at M = 128, 256, 512 and (b) the
    oracle's C transform (ora_bsk_to_fourier: fft_ld, its own pi and twiddles) for N = 1024, L = 3:
    every component within the sum of the two allowances (the direct sum's is (M + 3) eps sum|z|,
    the C transform's ld_allowance plus its rounding to double).

    Measured shares of components that differ after rounding to double (random 21/22-bit limb
    polynomials; the "tie-proximity rate" of two correct long-double results):
        spectrum_ld vs direct DFT       M = 128: 0.58 %   M = 256: 0.56 %   M = 512: 0.63 %
        spectrum_ld vs oracle fft_ld    N = 1024, L = 3 (49,152 components): 0.00 % (the same
                                        radix-2 schedule: its own pi and tables round identically)
        numpy f64 FFT vs spectrum_ld    M = 128: 75.7 %   M = 256: 76.8 %   M = 512: 78.0 %
                                        (worst element error 8.6 .. 10.1 u rms)
    K.LD_SHARE (0.7 %) and K.F64_SHARE (70 %) are these figures rounded away from each other; the
    GPU test's cap on a double-double format's share is 4 K.LD_SHARE = 2.8 % and must stay below
    K.F64_SHARE / 10 = 7 %."""
    rng = np.random.RandomState(13)
    shares = {}
    for M, polys in ((128, 64), (256, 32), (512, 16)):
        N = 2 * M
        g = rng.randint(-2 ** 21, 2 ** 21, size=(polys, N)).astype(np.int64)
        re, im = K.spectrum_ld(g, N)
        z = K.fold_twist(g, N)
        d = _direct_dft(z, M)
        zn = np.sqrt(np.sum(g.astype(np.float64) ** 2, axis=1))
        z1 = np.sum(np.abs(z), axis=1).astype(np.float64)
        tol = (K.ld_allowance(zn, M) + (M + 3) * EPS * z1)[:, None]
        assert np.all(np.abs(d.real - re) <= tol) and np.all(np.abs(d.imag - im) <= tol), M
        ld = _share(np.concatenate((d.real, d.imag)), np.concatenate((re, im)))
        f = np.fft.fft(z.astype(np.complex128), axis=1)
        f64 = _share(np.concatenate((f.real, f.imag)), np.concatenate((re, im)))
        worst = float(np.max(np.abs(np.concatenate((f.real - re, f.imag - im), axis=1)) / (U * zn[:, None] / np.sqrt(2))))
        print(f"M={M}: ld-vs-direct share {ld:.4%}, numpy f64 share {f64:.2%}, f64 worst {worst:.1f} u rms")
        shares[M] = (ld, f64)
        assert ld <= K.LD_SHARE and f64 >= K.F64_SHARE, (M, ld, f64)

    # (b) the C transform, through the limb split of bsk.hip's N = 1024 format
    p = oracle.Params(n=2, k=1, N=1024, l=1, logB=7, limbs=3)
    words = rng.randint(0, 2 ** 32, size=(8 * 1024, 2), dtype=np.int64)
    bsk = (words[:, 0].astype(np.uint64) << np.uint64(32)) | words[:, 1].astype(np.uint64)
    o = oracle.bsk_to_fourier(p, bsk).reshape(8, 3, 2, 512)  # [poly][limb][re / im][M], scaled 1/M
    lim = K.limbs_equal(bsk.reshape(8, 1024), 3)              # (3, 8, 1024)
    re, im = K.spectrum_ld(lim, 1024)
    zn = np.sqrt(np.sum(lim.astype(np.float64) ** 2, axis=-1))
    ref = np.stack((re, im), axis=2).transpose(1, 0, 2, 3) / LD(512)  # -> [poly][limb][re / im][M]
    tol = (2.0 * K.ld_allowance(zn, 512) / 512.0).T[:, :, None, None] + U * np.abs(ref).astype(np.float64)
    assert np.all(np.abs(o - ref) <= tol)
    c_share = _share(o, ref)
    print(f"N=1024 L=3: spectrum_ld vs oracle fft_ld share {c_share:.4%}")
    assert c_share <= K.LD_SHARE, c_share
    assert 4.0 * K.LD_SHARE <= K.F64_SHARE / 10.0


def test_mpmath_spot_check():
    """Extra, when mpmath is there: 16 frequencies of one M = 512 spectrum against a 200-bit sum."""
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 200
    rng = np.random.RandomState(14)
    N, M = 1024, 512
    g = rng.randint(-2 ** 21, 2 ** 21, size=N).astype(np.int64)
    re, im = K.spectrum_ld(g, N)
    zn = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    for f in rng.randint(0, M, size=16):
        acc = mp.mpc(0)
        for j in range(M):
            acc += mp.mpc(int(g[j]), int(g[j + M])) * mp.expjpi(mp.mpf(j - 4 * j * int(f)) / N)
        assert abs(float(mp.mpf(float(re[f])) + mp.mpf(float(re[f] - LD(float(re[f])))) - acc.real)) <= K.ld_allowance(zn, M)
        assert abs(float(mp.mpf(float(im[f])) + mp.mpf(float(im[f] - LD(float(im[f])))) - acc.imag)) <= K.ld_allowance(zn, M)


# ------------------------------------------------------------------------------------------
# index maps
# ------------------------------------------------------------------------------------------
MAP_SHAPES = [
    # (kind, k, N, l): every row of the GPU test's table, plus both orders of the level-major formats
    (K.KIND_N1024, 1, 1024, 1), (K.KIND_N1024, 1, 1024, 2), (K.KIND_N1024, 1, 1024, 3),
    (K.KIND_N2048, 1, 2048, 1), (K.KIND_N2048, 1, 2048, 2), (K.KIND_N2048, 1, 2048, 4),
    (K.KIND_K2N1024, 2, 1024, 1), (K.KIND_K2N1024, 2, 1024, 2), (K.KIND_K2N1024, 2, 1024, 3),
    (K.KIND_SMALL, 3, 512, 1), (K.KIND_SMALL, 3, 512, 3), (K.KIND_SMALL, 4, 512, 1), (K.KIND_SMALL, 4, 512, 2),
    (K.KIND_SMALL, 4, 512, 3), (K.KIND_SMALL, 5, 256, 1), (K.KIND_SMALL, 6, 256, 1),
    (K.KIND_GENERIC, 2, 512, 2), (K.KIND_GENERIC, 2, 256, 5), (K.KIND_GENERIC, 1, 4096, 1), (K.KIND_GENERIC, 1, 16384, 2),
    (K.KIND_GENERIC, 1, 32768, 1), (K.KIND_GENERIC, 1, 65536, 1),
]


@pytest.mark.parametrize("shape", MAP_SHAPES, ids=lambda s: "kind%d-k%d-N%d-l%d" % s)
def test_index_map_is_a_bijection_onto_the_key_buffer(shape):
    """Each layout's map names every (polynomial, limb, frequency[, +-]) exactly once and has as
    many elements as the key buffer (concrete_hip_fourier_bsk_size_bytes, whose closed forms the
    layout tests assert; no GPU needed) holds complex values."""
    from concrete_amd import backend as B
    kind, k, N, l = shape
    n = 1 if N >= 32768 else 2
    p = B.PbsParams(n=n, k=k, N=N, level=l, base_log=1, ks_level=1, ks_base_log=1)
    code, limbs, bits = B.bsk_format(p)
    assert code == kind and limbs > 0
    m = K.key_map(kind, n, k, N, l, limbs)
    assert m.limbs == limbs
    assert m.poly.size * 16 == B.fourier_bsk_bytes(p)
    if kind == K.KIND_GENERIC:
        from concrete_amd import _native
        assert m.poly.size * 16 == _native.lib().concrete_hip_generic_bsk_size_bytes(n, k, l, N)
        assert m.poly.size == n * (k + 1) ** 2 * l * limbs * (N // 2)
    npoly = n * l * (k + 1) ** 2
    mfreq = 512 if kind == K.KIND_N2048 else N // 2
    assert m.poly.min() == 0 and m.poly.max() == npoly - 1
    assert m.limb.min() == 0 and m.limb.max() == limbs - 1
    assert m.freq.min() == 0 and m.freq.max() == mfreq - 1
    key = (m.poly * limbs + m.limb) * mfreq + m.freq
    if m.pm is not None:
        key = key * 2 + m.pm
    assert key.size == npoly * limbs * mfreq * (2 if m.pm is not None else 1)
    assert np.unique(key).size == key.size


def test_frequency_orders():
    lane, slot = np.arange(64), np.arange(8)
    f = K.fft512_freq(lane[None, :], slot[:, None])
    assert sorted(f.reshape(-1)) == list(range(512)) and f[0, 1] == 8 and f[0, 8] == 1 and f[1, 0] == 64
    p = np.arange(32768)
    assert sorted(K.big_freq(p)) == list(range(32768))
    assert np.array_equal(K.big_freq(p[:512]), f.reshape(-1)) and K.big_freq(512 * 37 + 64 * 2 + 9) == 512 * 37 + 128 + 9
