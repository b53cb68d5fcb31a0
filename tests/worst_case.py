"""Worst-case inputs for the PBS and keyswitch kernels (numpy and the CPU oracle only).

The exactness arguments of DESIGN.md §3 are worst-case arguments: the f64 products are exact for
any digits with |d| <= 2^(logB-1) and any key with the measured max|G|, and the keyswitch's int32
partial sums cannot overflow for any digit row sum up to l 2^(logB-1).  Uniform random inputs stay
far from both.  This module builds the inputs that do not:

* words whose closest-representative decomposition has every level at its extreme
  (extreme_words), or whose l = 1 digit splits into the extreme sub-digits of the limb-grid kernels
  (subdigit_words);
* accumulators that put those words in front of one CMUX step (worst_accumulator, worst_batch);
* keys that are random except for one GGSW whose polynomials are a constant run (crafted_key), with
  the run length that puts max|G| where a test wants it (run_max_spectrum, run_for_spectrum).

Nothing here loads the HIP library, and nothing runs at import time; tests/test_worst_case_inputs.py
checks every claim made here against the oracle.
"""
import math

import numpy as np

MASK64 = (1 << 64) - 1
CRAFTED = 0x5555555555555555  # the constant key word of tests/test_gpu_robustness.py
FAMILIES = ("constant", "alternating")

# restated from concrete_amd/csrc/kernel_util.hpp (sub_digit_split) and pbs.hpp
SUB_BITS = 16


# ------------------------------------------------------------------------------------------
# digits
# ------------------------------------------------------------------------------------------
def extreme_fields(l, logB, sign):
    """The logB-bit field every level carries.  sign > 0: B/2 - 1, the digit itself.  sign < 0:
    B/2, which ora_decompose turns into -B/2 at the lowest level and, through the carry it sends up,
    into -(B/2 - 1) at every level above it; with one level there is no level above to decide the
    tie (a lone B/2 stays +B/2), so l = 1 takes B/2 + 1, the digit -(B/2 - 1)."""
    half = 1 << (logB - 1)
    if sign > 0:
        return half - 1
    return half if l > 1 else (half + 1) & ((1 << logB) - 1)


def extreme_words(l, logB, sign):
    """u64 words whose closest-representative decomposition has every level at the extreme of
    `sign` (+1 / -1): the field pattern of extreme_fields in the top l logB bits, and below it
    either zeros (an even word: -2 acc can take it) or the largest tail that still rounds down.
    l logB <= 63: the word needs a free low bit to be twice something."""
    assert l >= 1 and logB >= 1 and l * logB <= 63, (l, logB)
    field = extreme_fields(l, logB, sign)
    nrep = 64 - l * logB
    w = 0
    for q in range(l):
        w |= field << (nrep + q * logB)
    if logB == 1:
        # B/2 - 1 = 0: the closest representative in base 2 never has two neighbouring non-zero
        # digits, so the extreme is +-1 at every other level, ceil(l / 2) of them
        w = sum(1 << (nrep + q) for q in range(0, l, 2))
        if sign < 0:
            w = (-w) & MASK64
    words = [w]
    if nrep >= 2:
        words.append(w | ((1 << (nrep - 1)) - 1))
    return np.array(words, dtype=np.uint64)


def sub_digit_split(d):
    """kernel_util.hpp sub_digit_split on Python ints or int64 arrays: d = lo + 2^16 hi with lo
    balanced in [-2^15, 2^15)."""
    half = 1 << (SUB_BITS - 1)
    lo = ((d + half) & ((1 << SUB_BITS) - 1)) - half
    return lo, (d - lo) >> SUB_BITS


def subdigit_digit(logB, sign):
    """The l = 1 digit with d_lo = -2^15 and the largest |d_hi| of that sign the split can produce:
    +-(2^(logB-1) - 2^15), d_hi = 2^(logB-17) and -(2^(logB-17) - 1)."""
    assert logB >= SUB_BITS + 1
    return sign * ((1 << (logB - 1)) - (1 << (SUB_BITS - 1)))


def subdigit_words(logB, sign):
    """The even u64 word whose one digit (l = 1) is subdigit_digit(logB, sign)."""
    field = subdigit_digit(logB, sign) & ((1 << logB) - 1)
    return np.array([field << (64 - logB)], dtype=np.uint64)


def step_words(l, logB, words):
    """(positive, negative) even words of a word family: "extreme" or "subdigit" (l = 1)."""
    if words == "subdigit":
        assert l == 1
        return int(subdigit_words(logB, 1)[0]), int(subdigit_words(logB, -1)[0])
    assert words == "extreme", words
    return int(extreme_words(l, logB, 1)[0]), int(extreme_words(l, logB, -1)[0])


# ------------------------------------------------------------------------------------------
# one worst step
# ------------------------------------------------------------------------------------------
def step_signs(N, i0, family):
    """+1 for j <= i0 and -1 above it; the alternating family multiplies by (-1)^j."""
    assert family in FAMILIES and 0 <= i0 < N
    j = np.arange(N)
    s = np.where(j <= i0, 1, -1)
    return s * np.where(j & 1, -1, 1) if family == "alternating" else s


def worst_accumulator(k, N, l, logB, i0, family, words="extreme"):
    """A (k+1) N accumulator, every polynomial the same, whose rotation by N turns the CMUX input
    X^N acc - acc = -2 acc into the step pattern of extreme words: acc_j = -w_j / 2 mod 2^64."""
    wp, wn = step_words(l, logB, words)
    assert wp % 2 == 0 and wn % 2 == 0
    half = {1: ((-wp) & MASK64) >> 1, -1: ((-wn) & MASK64) >> 1}
    s = step_signs(N, i0, family)
    poly = np.where(s > 0, np.uint64(half[1]), np.uint64(half[-1])).astype(np.uint64)
    return np.tile(poly, k + 1)


def cmux_input(acc):
    """-2 acc mod 2^64: what the step after a rotation by N decomposes."""
    with np.errstate(over="ignore"):
        return (np.uint64(0) - acc) * np.uint64(2)


def rand_u64(rng, shape):
    return (rng.randint(0, 1 << 32, size=shape).astype(np.uint64) << np.uint64(32)) | \
        rng.randint(0, 1 << 32, size=shape).astype(np.uint64)


def batch_rows(N, batch):
    """(step, family, i0) of the worst-case rows of a batch: 8 of them for a batch of 9 ({step 0, step 1}
    x {constant, alternating} x {N/3, N-1}), 2 for the batch of 3 of the largest rings."""
    rows = [(step, fam, i0) for step in (0, 1) for fam in FAMILIES for i0 in (N // 3, N - 1)]
    if batch == 9:
        return rows
    assert batch == 3
    return [rows[0], rows[7]]  # (0, constant, N/3) and (1, alternating, N-1)


def worst_batch(k, N, l, logB, seed, batch=9, words="extreme"):
    """(ciphertexts (batch, 3), accumulators (batch, (k+1)N), lut_idx): n = 2, body 0, mask word 2^63 at
    the worst step and 0 at the other one (a rotation by 0: the accumulator reaches or leaves the
    worst step intact); the last row is uniform random, as a control.  words = "uniform": every row uniform
    random.  Read-only arrays."""
    rng = np.random.RandomState(seed)
    rows = batch_rows(N, batch) if words != "uniform" else []
    cts = np.zeros((batch, 3), dtype=np.uint64)
    accs = np.zeros((batch, (k + 1) * N), dtype=np.uint64)
    for r, (step, fam, i0) in enumerate(rows):
        cts[r, step] = np.uint64(1 << 63)
        accs[r] = worst_accumulator(k, N, l, logB, i0, fam, words)
    cts[batch - 1] = rand_u64(rng, 3)
    accs[batch - 1] = rand_u64(rng, (k + 1) * N)
    if words == "uniform":  # every row as the control row: what the worst-case residuals are compared with
        cts, accs = rand_u64(rng, cts.shape), rand_u64(rng, accs.shape)
    lut_idx = np.arange(batch, dtype=np.uint64)
    for a in (cts, accs, lut_idx):
        a.setflags(write=False)
    return cts, accs, lut_idx


# ------------------------------------------------------------------------------------------
# keys
# ------------------------------------------------------------------------------------------
def limb_widths(kind, limbs, bits):
    """Key limb widths of a device key format (concrete_hip_bsk_format's kind, limbs, bits)."""
    from oracle import keyref
    return keyref.generic_widths(bits, limbs) if kind == keyref.KIND_GENERIC else keyref.equal_widths(limbs)


def limb_extreme_word(widths):
    """The word whose every balanced limb is at its positive maximum 2^(w-1) - 1: 0x7FFF7FFF7FFF7FFF on
    the 16-bit grid."""
    w, shift = 0, 0
    for width in widths:
        w |= ((1 << (width - 1)) - 1) << shift
        shift += width
    assert shift == 64
    return w


def max_limb(word, widths):
    """max |limb| of a word (and of its negative, which the alternating family also plants)."""
    from oracle import keyref
    both = np.array([word & MASK64, (-word) & MASK64], dtype=np.uint64)
    return int(np.max(np.abs(keyref._balanced_split(both, widths))))


def crafted_key(k, N, l, n, step, family, m, word, seed):
    """A standard key [n][l][k+1][k+1][N] of uniform random words, except GGSW `step`: every row and
    column polynomial of every level is `word` on its first m coefficients (times (-1)^j for the
    alternating family, which moves the spectral peak from frequency 0 to N/4) and zero after."""
    assert 0 <= step < n and 1 <= m <= N and family in FAMILIES
    rng = np.random.RandomState(seed)
    key = rand_u64(rng, (n, l * (k + 1) ** 2, N))
    poly = np.zeros(N, dtype=np.uint64)
    poly[:m] = np.uint64(word & MASK64)
    if family == "alternating":
        poly[1:m:2] = np.uint64((-word) & MASK64)
    key[step] = poly
    return key.reshape(-1)


def run_max_spectrum(N, vmax, m):
    """max|G| of a limb polynomial that is +-vmax on its first m coefficients (constant or
    alternating): the folded, twisted transform evaluates the polynomial at odd 2N-th roots of unity, and
    the geometric sum peaks at the root nearest 1 (or -1): vmax sin(m pi / 2N) / sin(pi / 2N),
    increasing in m up to m = N."""
    return vmax * math.sin(m * math.pi / (2 * N)) / math.sin(math.pi / (2 * N))


def run_for_spectrum(N, vmax, target):
    """The smallest run length whose run_max_spectrum reaches `target`; None when the full run stays
    below it."""
    if run_max_spectrum(N, vmax, N) < target:
        return None
    x = min(1.0, target * math.sin(math.pi / (2 * N)) / vmax)
    m = max(1, min(N, int(math.ceil(2 * N / math.pi * math.asin(x)))))
    while m < N and run_max_spectrum(N, vmax, m) < target:
        m += 1
    return m


def static_gate_ok(kind, k, N, l, logB):
    """The hand-tuned kernels' static gates, restated from concrete_amd/csrc/pbs.hpp (pbs1024_exact,
    pbs2048_ok, k2_ok, pbs_small_ok) for the shapes that have such a kernel.  The ABI's
    concrete_hip_pbs_supported also admits the wider digits that the general path takes on a companion
    key, so it cannot say where a hand-tuned kernel's own range ends; the GPU tests tie this restatement
    to the library by calling one past the top with a key that has no companion."""
    from oracle import keyref
    whole = logB <= 15 and (l << (logB - 1)) <= (1 << 15)  # l whole digits on the 16-bit limb grid
    if logB < 1:
        return False
    if kind == keyref.KIND_N1024:
        return 1 <= l <= 3 and logB <= 11 and ((k + 1) * l << logB) <= 4096
    if kind == keyref.KIND_N2048:
        return logB <= 24 if l == 1 else (2 <= l <= 4 and whole)
    if kind == keyref.KIND_K2N1024:
        if l == 1:
            return logB <= 24
        return 2 <= l <= 64 and not (l >= keyref.K2_MANY_MIN and l * logB >= 64) and whole
    assert kind == keyref.KIND_SMALL, kind
    if l == 1:
        return logB <= 24
    if keyref.small_limbs(k, N, l) == keyref.K4_L2_LIMBS:
        return logB <= 16
    return l * logB < 64 and whole


# ------------------------------------------------------------------------------------------
# keyswitch
# ------------------------------------------------------------------------------------------
KS_KEY_WORDS = {
    "ones": 0xFFFFFFFFFFFFFFFF,     # every 22/21/21 and every 16-bit chunk at its maximum
    "i8min": 0x8080808080808080,    # every balanced int8 byte at -128
    "i8max": 0x7F7F7F7F7F7F7F7F,    # every balanced int8 byte at +127 (no carry between bytes)
}


def ks_inputs(n_in, l, logB, batch, seed):
    """(batch, n_in + 1) keyswitch inputs: rows cycle through all-negative-extreme, all-positive-extreme
    and a mix of both words' variants per position; the last row is uniform random."""
    rng = np.random.RandomState(seed)
    neg, pos = extreme_words(l, logB, -1), extreme_words(l, logB, 1)
    cts = np.empty((batch, n_in + 1), dtype=np.uint64)
    for r in range(batch - 1):
        if r % 3 == 0:
            cts[r] = neg[r // 3 % len(neg)]
        elif r % 3 == 1:
            cts[r] = pos[r // 3 % len(pos)]
        else:
            both = np.concatenate([neg, pos])
            cts[r] = both[rng.randint(0, len(both), size=n_in + 1)]
    cts[batch - 1] = rand_u64(rng, n_in + 1)
    cts.setflags(write=False)
    return cts


def ks_key(n_in, l, n_out, name, seed):
    """A keyswitch key [n_in][l][n_out + 1] of one extreme word, or uniform random words."""
    if name == "uniform":
        return rand_u64(np.random.RandomState(seed), n_in * l * (n_out + 1))
    return np.full(n_in * l * (n_out + 1), KS_KEY_WORDS[name], dtype=np.uint64)
