"""High-precision reference for every device Fourier key format.

TEST INFRASTRUCTURE ONLY (numpy alone): imported by tests/test_keyref.py, which shows that the
reference is right, and by tests/test_gpu_key_accuracy.py, which compares every stored element of
every key format with it.

The device converts each u64 key polynomial g into balanced signed limbs, and each limb polynomial
into the spectrum of the folded, twisted M = N/2 point transform

    z_j = (g_j + i g_{j+M}) exp(i pi j / N),     G_f = sum_j z_j exp(-2 pi i j f / M),

stored with a per-format scale and order (concrete_amd/csrc/bsk.hip, pbs_generic.hip).  Here the
same transform runs in np.longdouble (x87 extended, 64-bit significand) with twiddles whose angles
are reduced on integers and multiplied by a 64-bit pi, so the reference is about 2^11 times more
accurate than an f64 spectrum; ld_allowance bounds its error.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).nmant >= 63, "oracle/keyref.py needs an extended-precision long double"

# pi to 64 bits: the double nearest pi plus the double nearest the remainder (longdouble(np.pi) has
# only 53 bits and would put a 1e-16 relative error into every angle)
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)

# restated from concrete_amd/csrc/pbs.hpp
K2_LIMBS = 4
K2_MANY_MIN = 3    # k = 2, N = 1024: level-major key order from this level count
SM_LIMBS = 4
K4_L2_LIMBS = 5    # k = 4, N = 512, l = 2: five 13-bit limbs
K4_MANY_MIN = 3    # k = 4, N = 512: level-major key order from this level count
SM_GC256 = 2       # N = 256 key groups hold two output columns when k + 1 is even
PBS2_LIMBS = 4

KIND_N1024, KIND_N2048, KIND_GENERIC, KIND_K2N1024, KIND_SMALL = 1, 2, 3, 4, 5  # concrete_hip_bsk_format

# Shares of components that differ after rounding to double, measured on the CPU by
# tests/test_keyref.py::test_independent_long_double_transforms_agree, which asserts both: two
# correct long-double transforms of one input differ in at most LD_SHARE of the components (a value
# near a rounding tie), numpy's f64 FFT differs from the long-double one in at least F64_SHARE.
LD_SHARE = 0.007
F64_SHARE = 0.70


# ------------------------------------------------------------------------------------------
# limb splits
# ------------------------------------------------------------------------------------------
def _words(words) -> np.ndarray:
    if isinstance(words, np.ndarray):
        return words.astype(np.uint64, copy=False)
    if isinstance(words, (list, tuple)):
        return np.array([int(w) & 0xFFFFFFFFFFFFFFFF for w in words], dtype=np.uint64)
    return np.array(int(words) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


def equal_widths(L: int) -> list[int]:
    """Limb widths of bsk.hip's limb_value<LIMBS>: 64 / L, the first 64 % L one bit wider."""
    return [64 // L + (1 if t < 64 % L else 0) for t in range(L)]


def _balanced_split(words, widths) -> np.ndarray:
    """x = sum_t limb_t 2^{s_t} (mod 2^64), limb_t in [-2^(w_t-1), 2^(w_t-1)): a value >= 2^(w-1)
    is negative, and the limb is subtracted before the shift (the carry moves up)."""
    rem = _words(words).copy()
    out = np.empty((len(widths),) + rem.shape, dtype=np.int64)
    for t, w in enumerate(widths):
        if w >= 64:  # one 64-bit limb: the signed reading of the word
            out[t] = rem.view(np.int64) if rem.ndim else rem.astype(np.int64)
            rem = np.zeros_like(rem)
            continue
        vv = rem & np.uint64((1 << w) - 1)
        sgn = vv.astype(np.int64) - np.where(vv >= np.uint64(1 << (w - 1)), np.int64(1) << np.int64(w), np.int64(0))
        out[t] = sgn
        with np.errstate(over="ignore"):
            rem = (rem - sgn.astype(np.uint64)) >> np.uint64(w)
    return out


def limbs_equal(words, L: int) -> np.ndarray:
    """Balanced limbs of the hand-tuned formats (bsk.hip: limb_value<LIMBS>), int64, shape
    (L,) + words.shape."""
    return _balanced_split(words, equal_widths(L))


def generic_widths(bits: int, L: int) -> list[int]:
    return [bits] * (L - 1) + [64 - (L - 1) * bits]


def generic_limb_bits(k: int, N: int, l: int) -> int:
    """Limb width of the general format of (k, N, l), restating pbs_generic.hip:generic_limb_bits on
    the oracle's generic_error_bound (a companion key's width is not reported by the ABI; for the
    shapes whose own format is the general one, concrete_hip_bsk_format is, and the tests compare)."""
    from oracle.pyoracle import generic_error_bound
    for b in range(24, 7, -1):
        if generic_error_bound(k, N, l, min(2 * b, 64 // l), b) < 0.25:
            return b
    return 0


def limbs_generic(words, bits: int, L: int) -> np.ndarray:
    """Balanced limbs of the general format (pbs_generic.hip: gen_convert_kernel): L - 1 limbs of
    `bits` bits and the top limb balanced in its own width 64 - (L - 1) bits; int64, shape
    (L,) + words.shape."""
    assert 0 < 64 - (L - 1) * bits <= bits
    return _balanced_split(words, generic_widths(bits, L))


# ------------------------------------------------------------------------------------------
# the long-double transform
# ------------------------------------------------------------------------------------------
def cis_ld(num, den: int) -> np.ndarray:
    """exp(i pi num / den) for integer num (array or scalar): the angle is reduced on integers to
    (-den, den] before it meets pi."""
    r = np.asarray(num, dtype=np.int64) % (2 * den)
    r = np.where(r > den, r - 2 * den, r)
    ang = PI_LD * r.astype(LD) / LD(den)
    out = np.empty(r.shape, dtype=CLD)
    out.real = np.cos(ang)
    out.imag = np.sin(ang)
    return out


_TABLES: dict[int, tuple] = {}


def _tables(N: int):
    """(twist zeta^j = exp(i pi j / N), j < M; twiddles exp(-2 pi i t / M), t < M / 2; bit reversal)"""
    if N not in _TABLES:
        M = N // 2
        logm = M.bit_length() - 1
        assert 1 << logm == M and M >= 2
        j = np.arange(M, dtype=np.int64)
        rev = np.zeros(M, dtype=np.int64)
        for b in range(logm):
            rev |= ((j >> b) & 1) << (logm - 1 - b)
        _TABLES[N] = (cis_ld(j, N), cis_ld(-2 * np.arange(M // 2, dtype=np.int64), M), rev)
    return _TABLES[N]


def fold_twist(limb_poly, N: int) -> np.ndarray:
    """z_j = (g_j + i g_{j+M}) exp(i pi j / N), clongdouble, shape (..., M)."""
    g = np.asarray(limb_poly)
    assert g.shape[-1] == N
    M = N // 2
    z = np.empty(g.shape[:-1] + (M,), dtype=CLD)
    z.real = g[..., :M].astype(LD)
    z.imag = g[..., M:].astype(LD)
    return z * _tables(N)[0]


def spectrum_ld(limb_poly, N: int):
    """Unnormalised forward spectrum G_f = sum_j z_j exp(-2 pi i j f / M) of the folded, twisted
    limb polynomial(s) (..., N), in natural frequency order: (real, imaginary) long-double arrays
    of shape (..., M).  Vectorised radix-2 decimation in time."""
    M = N // 2
    _, tw, rev = _tables(N)
    x = fold_twist(limb_poly, N)[..., rev]
    lead = x.shape[:-1]
    half = 1
    while half < M:
        x = x.reshape(lead + (M // (2 * half), 2, half))
        u = x[..., 0, :]
        v = x[..., 1, :] * tw[:: M // (2 * half)]
        x = np.stack((u + v, u - v), axis=-2)
        half *= 2
    x = x.reshape(lead + (M,))
    return np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)


def ld_allowance(z_norm2, M: int):
    """Higham's FFT bound (Accuracy and Stability, Thm 24.2) at unit roundoff eps = 2^-64 with
    twiddles accurate to eps: the 2-norm error of an M-point long-double spectrum of z (and so of
    each of its elements) is at most gamma sqrt(M) ||z||_2."""
    eps = 2.0 ** -64
    eta = eps + 4.0 * eps * (np.sqrt(2.0) + eps) / (1.0 - 4.0 * eps)
    logm = float(np.log2(M))
    gamma = logm * eta / (1.0 - logm * eta)
    return gamma * np.sqrt(float(M)) * z_norm2


def gamma_generic(M: int) -> float:
    """gamma of the general path's f64 transforms, exactly as pyoracle.generic_error_bound: twiddle
    error mu = 5u, 2 log2 M stages."""
    u = 2.0 ** -53
    mu = 5.0 * u
    eta = mu + 4.0 * u / (1.0 - 4.0 * u) * (np.sqrt(2.0) + mu)
    logm = float(np.log2(M))
    return 2.0 * logm * eta / (1.0 - 2.0 * logm * eta)


# ------------------------------------------------------------------------------------------
# index maps: which (standard polynomial, limb, frequency) each stored complex element holds
# ------------------------------------------------------------------------------------------
def fft512_freq(lane, slot):
    """Frequency held by (lane, slot) of the one-wave transforms' register layout (fft512.hpp)."""
    return (lane >> 3) + 8 * (lane & 7) + 64 * slot


def big_freq(p):
    """Frequency at position p of the four-step order (pbs_generic.hip): position k1 512 + slot 64 +
    lane holds frequency fft512_freq(lane, slot) + 512 k1.  The split conversion at N >= 32768
    (gen_split_combine_kernel: p >> 9 = k1 < R, p & 511 = the class transforms' position) stores
    the same order with more rows."""
    return fft512_freq(p & 63, (p >> 6) & 7) + 512 * (p >> 9)


@dataclass
class KeyMap:
    """Per stored complex element, flat in buffer order: the standard polynomial index
    ((i l + v) (k+1) + row) (k+1) + col of the input layout [n][l][row][col][N], the limb, the
    frequency, and for the N2048 format which of K+ (0) / K- (1) it is.  `scale` multiplies the
    unnormalised spectrum; m_eff is the transform length the element belongs to."""
    poly: np.ndarray
    limb: np.ndarray
    freq: np.ndarray
    pm: np.ndarray | None
    scale: float
    m_eff: int
    limbs: int


def _grid(*dims):
    return [a.reshape(-1) for a in np.indices(dims, dtype=np.int64)]


def _std_poly(i, q, row, col, k1, l):
    return ((i * l + (l - 1 - q)) * k1 + row) * k1 + col  # level v = l - 1 - q


def map_n1024(n: int, l: int) -> KeyMap:
    """k = 1, N = 1024, l <= 3 (bsk.hip: convert_bsk_kernel): [n][limb 3][co][ro][q][slot 8][lane 64];
    slots 0..3 of group (limb, co, ro) hold column co / row ro, slots 4..7 the "other" column
    1 - co / row 1 - ro; scale 1/512."""
    i, limb, co, ro, q, slot, lane = _grid(n, 3, 2, 2, l, 8, 64)
    own = slot < 4
    row, col = np.where(own, ro, 1 - ro), np.where(own, co, 1 - co)
    return KeyMap(_std_poly(i, q, row, col, 2, l), limb, fft512_freq(lane, slot), None, 1.0 / 512.0, 512, 3)


def map_n2048(n: int, l: int) -> KeyMap:
    """k = 1, N = 2048 (bsk.hip: convert_bsk2048_kernel, P2_PM): [n][limb 4][col][q][row][+-][slot 8]
    [lane 64], K+- = (G_e +- s_f G_o) / 2 of the two parity halves' 512-point spectra, stored / 512:
    the 1024-point negacyclic spectrum of the whole polynomial at +-s_f, scale 1/1024."""
    i, limb, col, q, row, pm, slot, lane = _grid(n, PBS2_LIMBS, 2, l, 2, 2, 8, 64)
    return KeyMap(_std_poly(i, q, row, col, 2, l), limb, fft512_freq(lane, slot), pm, 1.0 / 1024.0, 1024,
                  PBS2_LIMBS)


def map_k2n1024(n: int, l: int) -> KeyMap:
    """k = 2, N = 1024 (bsk.hip: convert_bsk1024k2_kernel): [n][limb 4][col 3][q][row 3][512], from
    l = K2_MANY_MIN level-major [n][q][limb][col][row][512]; scale 1/512."""
    if l >= K2_MANY_MIN:
        i, q, limb, col, row, e = _grid(n, l, K2_LIMBS, 3, 3, 512)
    else:
        i, limb, col, q, row, e = _grid(n, K2_LIMBS, 3, l, 3, 512)
    return KeyMap(_std_poly(i, q, row, col, 3, l), limb, fft512_freq(e & 63, e >> 6), None, 1.0 / 512.0, 512,
                  K2_LIMBS)


def small_limbs(k: int, N: int, l: int) -> int:
    return K4_L2_LIMBS if (N == 512 and k == 4 and l == 2) else SM_LIMBS


def sm_gc(N: int, k1: int) -> int:
    return SM_GC256 if (N == 256 and k1 % SM_GC256 == 0) else 1


def map_small(n: int, k: int, N: int, l: int) -> KeyMap:
    """N = 512, k = 3 / 4 and N = 256, k = 5 / 6 (bsk.hip: convert_bsk_small_kernel): key groups
    [n][limb][cg][q][c2][row][N/2] with col = cg GC + c2, GC = sm_gc(N, k + 1); k = 4, N = 512 from
    l = K4_MANY_MIN level-major [n][q][limb][col][row][N/2]; scale 1 / (512 P), P = 1024 / N."""
    k1, M, L = k + 1, N // 2, small_limbs(k, N, l)
    if N == 512 and k == 4 and l >= K4_MANY_MIN:
        i, q, limb, col, row, e = _grid(n, l, L, k1, k1, M)
    else:
        gc = sm_gc(N, k1)
        i, limb, cg, q, c2, row, e = _grid(n, L, k1 // gc, l, gc, k1, M)
        col = cg * gc + c2
    return KeyMap(_std_poly(i, q, row, col, k1, l), limb, fft512_freq(e & 63, e >> 6), None,
                  1.0 / (512.0 * (1024 // N)), M, L)


def map_generic(n: int, k: int, N: int, l: int, limbs: int) -> KeyMap:
    """General format (pbs_generic.hip: gen_convert_kernel, gen_split_combine_kernel):
    [n][col][limb][row][q][M], scale 1/M; natural frequency order below N = 2048, position p holds
    frequency big_freq(p) from N = 2048 (four-step order; the split conversion at N >= 32768 too)."""
    k1, M = k + 1, N // 2
    i, col, limb, row, q, p = _grid(n, k1, limbs, k1, l, M)
    return KeyMap(_std_poly(i, q, row, col, k1, l), limb, p if N < 2048 else big_freq(p), None, 1.0 / M, M, limbs)


def key_map(kind: int, n: int, k: int, N: int, l: int, limbs: int) -> KeyMap:
    if kind == KIND_N1024:
        return map_n1024(n, l)
    if kind == KIND_N2048:
        return map_n2048(n, l)
    if kind == KIND_K2N1024:
        return map_k2n1024(n, l)
    if kind == KIND_SMALL:
        return map_small(n, k, N, l)
    assert kind == KIND_GENERIC
    return map_generic(n, k, N, l, limbs)


# ------------------------------------------------------------------------------------------
# the reference key
# ------------------------------------------------------------------------------------------
@dataclass
class RefKey:
    """The long-double key in device order with the stored scale applied (re, im: flat long
    double), per element the 2-norm ||z||_2 = ||limb polynomial||_2 of the transform it belongs to,
    and the map."""
    re: np.ndarray
    im: np.ndarray
    znorm: np.ndarray
    map: KeyMap

    @property
    def max_spectrum(self) -> float:
        """max |G| over the whole key, unscaled (what concrete_hip_key_spectrum_max records)."""
        return float(np.max(np.hypot(self.re, self.im))) / self.map.scale

    @property
    def argmax_poly_limb(self):
        a = int(np.argmax(np.hypot(self.re, self.im)))
        return int(self.map.poly[a]), int(self.map.limb[a])


def reference_key(kind: int, words, n: int, k: int, N: int, l: int, limbs: int, bits: int) -> RefKey:
    """Reference of the device key of format `kind` for the standard key `words` ([n][l][row][col][N]
    u64): one long-double transform per (polynomial, limb), gathered through the format's map."""
    m = key_map(kind, n, k, N, l, limbs)
    npoly = n * l * (k + 1) ** 2
    g = _words(np.asarray(words)).reshape(npoly, N)
    lim = limbs_generic(g, bits, limbs) if kind == KIND_GENERIC else limbs_equal(g, limbs)  # (L, npoly, N)
    znorm = np.sqrt(np.sum(lim.astype(LD) ** 2, axis=-1)).astype(np.float64)               # (L, npoly)
    if kind == KIND_N2048:
        # parity halves p(u) = g[2u + par] as N = 1024 negacyclic polynomials; K+- in long double
        er, ei = spectrum_ld(lim[..., 0::2], 1024)
        orr, oi = spectrum_ld(lim[..., 1::2], 1024)
        ge = np.empty(er.shape, dtype=CLD)
        ge.real, ge.imag = er, ei
        go = np.empty(er.shape, dtype=CLD)
        go.real, go.imag = orr, oi
        so = go * cis_ld(1 - 4 * np.arange(512, dtype=np.int64), 2048)  # s_f = exp(i pi (1 - 4 f) / 2048)
        kpm = np.stack((ge + so, ge - so), axis=0)                     # G(+-s_f) = 2 K+-: (2, L, npoly, 512)
        val = kpm[m.pm, m.limb, m.poly, m.freq] * LD(m.scale)
    else:
        sr, si = spectrum_ld(lim, N)
        val = np.empty(m.poly.shape, dtype=CLD)
        val.real = sr[m.limb, m.poly, m.freq] * LD(m.scale)
        val.imag = si[m.limb, m.poly, m.freq] * LD(m.scale)
    return RefKey(np.ascontiguousarray(val.real), np.ascontiguousarray(val.imag), znorm[m.limb, m.poly], m)
