"""CPU checks of the worst-case inputs (tests/worst_case.py) that tests/test_gpu_worst_case.py runs: the
conditions that keep those GPU tests from being vacuous, against the oracle alone.  The HIP library is loaded
only inside test bodies (for the gates it exports), never at import.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_worst_case as G  # noqa: E402
import worst_case as W  # noqa: E402

# every (l, logB) the GPU lists decompose at, and the pairs the construction was first tried on
ISSUE_PAIRS = [(3, 7), (1, 23), (2, 15), (1, 11), (4, 9), (6, 7), (2, 16)]
PBS_PAIRS = sorted({(c[3], c[4]) for c in G.PBS_CASES})
KS_PAIRS = sorted({c[:2] for c in G.KS_VALU_CASES} | {c[1:3] for c in G.KS_MFMA_CASES})


def digits_of(oracle, words, l, logB):
    return np.array([oracle.decompose(w, l, logB) for w in np.asarray(words).reshape(-1)], dtype=np.int64)


@pytest.mark.parametrize("pair", sorted(set(ISSUE_PAIRS + PBS_PAIRS + KS_PAIRS)), ids=lambda p: "l%db%d" % p)
def test_extreme_words_decompose_to_extreme_digits(oracle, pair):
    """ora_decompose of every variant: all levels +(B/2 - 1); or -B/2 at the lowest level (the carry then
    crosses every level above it) and -(B/2 - 1) above; one level alone: -(B/2 - 1).  Base 2 has no such
    words (B/2 - 1 = 0, and no two neighbouring digits are non-zero): there every other level is +-1."""
    l, logB = pair
    half = 1 << (logB - 1)
    pos, neg = W.extreme_words(l, logB, 1), W.extreme_words(l, logB, -1)
    assert pos[0] % 2 == 0 and neg[0] % 2 == 0  # -2 acc can take the first variant
    dp, dn = digits_of(oracle, pos, l, logB), digits_of(oracle, neg, l, logB)
    if logB == 1:
        want = np.array([1 if q % 2 == 0 else 0 for q in range(l)])
        assert (dp == want).all() and (dn == -want).all()
        return
    assert (dp == half - 1).all()
    if l == 1:
        assert (dn == -(half - 1)).all()
    else:
        assert (dn[:, 0] == -half).all() and (dn[:, 1:] == -(half - 1)).all()
    assert np.abs(dp).mean() >= half - 1 and np.abs(dn).mean() >= half - 1


@pytest.mark.parametrize("logB", sorted({c[4] for c in G.PBS_CASES if c[6].get("words") == "subdigit"}))
def test_subdigit_words_reach_both_sub_digit_maxima(oracle, logB):
    """sub_digit_split restated: over every digit one level can produce, (-B/2, B/2], d_lo is never below -2^15
    and d_hi never above 2^(logB-17) (pbs.hpp allows one more); the sub-digit words' digits have d_lo = -2^15
    together with d_hi = 2^(logB-17), and with -(2^(logB-17) - 1), the most negative d_hi that goes with it."""
    half = 1 << (logB - 1)
    d = np.arange(-half + 1, half + 1, dtype=np.int64)
    lo, hi = W.sub_digit_split(d)
    assert (lo + (hi << 16) == d).all()
    assert lo.min() == -(1 << 15) and lo.max() == (1 << 15) - 1
    top = 1 << (logB - 17)
    assert hi.max() == top and hi.min() == -top and top <= (1 << (logB - 17)) + 1
    assert hi[lo == -(1 << 15)].max() == top and hi[lo == -(1 << 15)].min() == -(top - 1)
    for sign, want_hi in ((1, top), (-1, -(top - 1))):
        (digit,) = oracle.decompose(W.subdigit_words(logB, sign)[0], 1, logB)
        assert digit == W.subdigit_digit(logB, sign)
        assert W.sub_digit_split(digit) == (-(1 << 15), want_hi)


@pytest.mark.parametrize("case", G.PBS_CASES, ids=G.case_id)
def test_worst_step_input_is_extreme(oracle, case):
    """The CMUX input of the worst step, -2 acc, of every worst-case row of every case: mean |digit| >= B/2 - 1,
    the sign pattern is the step (times (-1)^j for the alternating family), and the negative words carry
    through every level (their lowest digit is -B/2)."""
    _, k, N, l, logB, _, opts = case
    words = opts.get("words", "extreme")
    half = 1 << (logB - 1)
    cts, accs, lut_idx = W.worst_batch(k, N, l, logB, 1, opts.get("batch", 9), words)
    rows = W.batch_rows(N, len(cts))
    assert len(cts) == len(rows) + 1 and (lut_idx == np.arange(len(cts))).all()
    for r, (step, family, i0) in enumerate(rows):
        assert cts[r].tolist() == [1 << 63 if s == step else 0 for s in (0, 1)] + [0]
        assert oracle.lib().ora_modswitch(int(cts[r, step]), N) == N  # a rotation by N: X^N acc = -acc
        x = W.cmux_input(accs[r])
        uniq, inv = np.unique(x, return_inverse=True)
        assert len(uniq) == (1 if (family, i0) == ("constant", N - 1) else 2)
        dig = digits_of(oracle, uniq, l, logB)[inv]  # (k+1)N x l
        if words == "subdigit":
            lo, hi = W.sub_digit_split(dig[:, 0])
            assert (lo == -(1 << 15)).all() and hi.max() == 1 << (logB - 17)
            assert np.abs(dig).mean() >= half - (1 << 15)
        else:
            assert np.abs(dig).mean() >= half - 1
            if l > 1:
                assert (dig[dig[:, 0] < 0, 0] == -half).all()  # the carry crosses every level
        sign = np.tile(W.step_signs(N, i0, family), k + 1)
        assert (np.sign(dig[:, -1]) == sign).all()
        assert (accs[r].reshape(k + 1, N) == accs[r, :N]).all()


@pytest.mark.parametrize("shape", [(1, 1024, 3, 7), (1, 2048, 1, 23), (2, 1024, 2, 15)], ids=lambda s: "k%dN%dl%db%d" % s)
def test_oracle_residual_on_the_worst_batch(oracle, shape):
    """The oracle's certified FFT path on the worst-case batch with the constant 0x5555... key: equal to its
    integer Karatsuba path word for word, with a rounding residual at least 8 times that of uniform
    accumulators with a uniform key at the same parameters (30 to 32 times was measured; the factor of four
    is for other seeds).  A condition on the inputs: the oracle alone computes it."""
    O = oracle
    k, N, l, logB = shape
    op = O.Params(n=2, k=k, N=N, l=l, logB=logB, limbs=O.limbs_for(N))
    cts, accs, lut_idx = W.worst_batch(k, N, l, logB, 11)
    key = np.full(op.n * l * (k + 1) ** 2 * N, W.CRAFTED, dtype=np.uint64)
    got, worst = O.pbs_batch(op, cts, accs, bsk=key, fbsk=O.bsk_to_fourier(op, key), lut_idx=lut_idx, mode=O.MODE_FFT)
    ref, _ = O.pbs_batch(op, cts, accs, bsk=key, lut_idx=lut_idx, mode=O.MODE_KARATSUBA)
    assert np.array_equal(got, ref)
    rng = np.random.RandomState(12)
    ukey, uaccs = W.rand_u64(rng, key.size), W.rand_u64(rng, accs.shape)
    ugot, uniform = O.pbs_batch(op, cts, uaccs, bsk=ukey, fbsk=O.bsk_to_fourier(op, ukey), lut_idx=lut_idx,
                                mode=O.MODE_FFT)
    uref, _ = O.pbs_batch(op, cts, uaccs, bsk=ukey, lut_idx=lut_idx, mode=O.MODE_KARATSUBA)
    assert np.array_equal(ugot, uref)
    print(f"k{k} N{N} l{l} logB{logB}: worst-case residual {worst:.3e}, uniform {uniform:.3e}, x{worst / uniform:.1f}")
    assert worst < 0.5 and worst >= 8.0 * uniform, (worst, uniform)


@pytest.mark.parametrize("case", G.PBS_CASES, ids=G.case_id)
def test_every_logb_is_at_the_top_of_its_gate(case):
    """Each literal logB is the largest its case can take, for the reason its `top` tag names.  The library is
    asked wherever it can answer: concrete_hip_pbs_supported admits logB; for a shape whose own format is the
    general one (and for the general path's companions) it refuses logB + 1.  A hand-tuned kernel's own range
    ends below what concrete_hip_pbs_supported admits (wider digits run on the general path), so there the
    restated gate (worst_case.static_gate_ok) decides, and the GPU test shows that one past it the kernel does
    not run."""
    from concrete_amd import _native
    from oracle import keyref
    L = _native.lib()
    _, k, N, l, logB, top, opts = case
    limbs, bits = C.c_uint32(), C.c_uint32()
    kind = L.concrete_hip_bsk_format(k, N, l, C.byref(limbs), C.byref(bits))
    generic = kind == keyref.KIND_GENERIC or opts.get("route") == "generic"
    gen_bits = bits.value if kind == keyref.KIND_GENERIC else keyref.generic_limb_bits(k, N, l)
    assert L.concrete_hip_pbs_supported(k, N, l, logB) == 1
    assert l * logB <= 63
    if top == "gate":
        if generic:
            assert L.concrete_hip_pbs_supported(k, N, l, logB + 1) == 0
        else:
            assert W.static_gate_ok(kind, k, N, l, logB) and not W.static_gate_ok(kind, k, N, l, logB + 1)
    elif top == "whole":
        assert l == 1 and logB == 15 and kind in (keyref.KIND_K2N1024, keyref.KIND_SMALL, keyref.KIND_N2048)
    elif top == "t2":
        assert generic and logB == 2 * gen_bits  # T = ceil(logB / bits) = 2; 3 from logB + 1
    elif top == "even":
        assert generic and l * (logB + 1) == 64 and L.concrete_hip_pbs_supported(k, N, l, logB + 1) == 1
        assert L.concrete_hip_pbs_supported(k, N, l, logB + 2) == 0
    else:
        assert top == "flagship" and (k, N, l, logB) in ((1, 1024, 3, 7), (1, 2048, 1, 23))
        assert W.static_gate_ok(kind, k, N, l, logB + 1)


@pytest.mark.parametrize("fmt", [
    # (kind, k, N, l, limbs, bits)
    (1, 1, 1024, 1, 3, 22), (2, 1, 2048, 1, 4, 16), (4, 2, 1024, 1, 4, 16), (5, 4, 512, 2, 5, 13), (3, 1, 4096, 1, 5, 13),
], ids=lambda f: "kind%d" % f[0])
def test_run_spectrum_formula_matches_the_long_double_key(fmt):
    """run_max_spectrum, which chooses the planted run's length, against oracle/keyref.py's long-double key
    of a GGSW whose polynomials are that run: constant and alternating, the 0x5555... word and the format's
    limb-extreme word, a short, a middling and the full run."""
    from oracle import keyref
    kind, k, N, l, limbs, bits = fmt
    widths = W.limb_widths(kind, limbs, bits)
    extreme = W.limb_extreme_word(widths)
    if bits == 16:
        assert extreme == 0x7FFF7FFF7FFF7FFF
    assert (keyref._balanced_split(np.array([extreme], dtype=np.uint64), widths)[:, 0] ==
            [(1 << (w - 1)) - 1 for w in widths]).all()
    for word in (W.CRAFTED, extreme):
        vmax = W.max_limb(word, widths)
        for family in W.FAMILIES:
            for m in (1, N // 3, N):
                key = W.crafted_key(k, N, l, 1, 0, family, m, word, 5)
                got = keyref.reference_key(kind, key, 1, k, N, l, limbs, bits).max_spectrum
                want = W.run_max_spectrum(N, vmax, m)
                assert abs(got / want - 1.0) < 1e-9, (hex(word), family, m, got, want)
                assert W.run_for_spectrum(N, vmax, want * (1 - 1e-12)) == m
    assert W.run_for_spectrum(N, vmax, 2.0 * W.run_max_spectrum(N, vmax, N)) is None


@pytest.mark.parametrize("case", G.KS_VALU_CASES + [(c[1], c[2], c[1] << (c[2] - 1), -1) for c in G.KS_MFMA_CASES],
                         ids=lambda c: "l%db%d" % c[:2])
def test_keyswitch_rows_reach_the_digit_row_sum(oracle, case):
    """The keyswitch inputs' extreme rows: every position's digit row sum is l (B/2 - 1) at least, within l of
    the dmax = l 2^(logB-1) that picks the kernel's form (base 2: ceil(l / 2), all a closest representative
    can carry); the literal dmax values sit at 32 and 1024 and one past each."""
    l, logB, dmax, nch = case
    assert dmax == l << (logB - 1)
    if nch >= 0:
        assert dmax in (32, 64, 1024, 2048) and nch == (3 if dmax <= 32 else 4 if dmax <= 1024 else 0)
    cts = W.ks_inputs(40, l, logB, 7, 3)
    floor = -(-l // 2) if logB == 1 else l * ((1 << (logB - 1)) - 1)
    for r in range(6):
        sums = np.abs(digits_of(oracle, cts[r], l, logB)).sum(axis=1)
        assert sums.min() >= floor and sums.max() <= dmax
    neg = digits_of(oracle, cts[0], l, logB)
    assert (neg <= 0).all() and (digits_of(oracle, cts[1], l, logB) >= 0).all()
    for name, word in W.KS_KEY_WORDS.items():
        assert (W.ks_key(3, l, 4, name, 0) == np.uint64(word)).all()
