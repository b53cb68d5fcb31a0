"""GPU tests of the slot-split cfg2 kernel's integer path (pbs1024_pair_slot_kernel<BL>,
concrete_amd/csrc/pbs.hip): base_log 7 runs the instance with the base fixed at
compile time (rot_word, decomp_word_digit, fixed_limb_add), base_log 6 and 5 the instance that
reads the base at run time, selected by the same launcher.  The kernel is forced with
CONCRETE_HIP_PBS_SLOT=1 on n = 12 (the step loop of n = 630); every output word must equal the
oracle's integer (Karatsuba) PBS.

Row 0 of every batch is set by hand:
  * its mask words modulus-switch to 1, 0 (the word 0, which the reference skips, and a nonzero word
    that rounds to 0), 2N - 1 and N, its body to 0: the edges of the rotation;
  * its accumulator is a full GLWE (both polynomials set) built so that ct1 of the first step,
    X acc - acc, holds chosen words: decomposer states whose level-0 and level-1 fields equal B/2 with
    the tie bit (the next field's top bit) clear and set, reached directly and through a carry, and
    the last level's field at B/2.  That this happens is asserted on the CPU with the oracle's own
    decomposition: a digit +B/2 is a tie with the bit clear, a digit -B/2 a tie with the bit set.
"""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

from test_gpu_pbs import B, Setup, encrypt, lut_acc, run_gpu, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

N, L, NB = 1024, 3, 9
BASES = (7, 6, 5)
BATCHES = (1, 4, 5, 9)


def tie_states(logB):
    """Decomposer states (l = 3) that reach each tie case; `half` = B/2."""
    half, Bs = 1 << (logB - 1), 1 << logB
    return [
        half,                                           # level 0 tie, bit clear -> +B/2
        half | half << logB,                            # level 0 tie, bit set   -> -B/2, carry
        half << logB,                                   # level 1 tie, bit clear
        half << logB | half << 2 * logB,                # level 1 tie, bit set
        (Bs - 1) | (half - 1) << logB,                  # carry from level 0 makes level 1's field B/2, bit clear
        (Bs - 1) | (half - 1) << logB | half << 2 * logB,  # the same with the bit set
        half << 2 * logB,                               # last level at B/2 (no bit above it)
        (Bs - 1) | (Bs - 1) << logB | (Bs - 1) << 2 * logB,  # carries through every level (state wraps to 2^(3 logB))
    ]


def crafted_acc(logB, rng):
    """A GLWE accumulator whose first-step ct1 = X acc - acc holds tie_states() (both polynomials)."""
    nrep = 64 - L * logB
    acc = np.zeros(2 * N, dtype=np.uint64)
    for p in range(2):
        target = rng.randint(0, 1 << 32, size=N).astype(np.uint64) << np.uint64(32)
        target |= rng.randint(0, 1 << 32, size=N).astype(np.uint64)
        for i, st in enumerate(tie_states(logB)):
            for rep in range(4):  # several lanes and register slots of the wave
                j = 1 + 64 * ((3 * i + 5 * rep + p) % 16) + (7 * i + 13 * rep) % 63
                # the state's word, with low bits that round down (below 2^(nrep-1)) or are empty
                low = int(rng.randint(0, 1 << 20)) if rep % 2 else 0
                target[j] = np.uint64(((st << nrep) + low) & (2 ** 64 - 1))
        # ct1[j] = acc[j - 1] - acc[j] for j >= 1: acc by running differences
        a = np.zeros(N, dtype=np.uint64)
        a[0] = np.uint64(int(rng.randint(0, 1 << 31)) << 33)
        with np.errstate(over="ignore"):
            for j in range(1, N):
                a[j] = a[j - 1] - target[j]
        acc[p * N:(p + 1) * N] = a
    return acc


def first_step_digits(oracle, acc, logB, a_t):
    """The oracle's digits of ct1 = X^{a_t} acc - acc, shape (2, N, L)."""
    lib = oracle.lib()
    out = np.zeros((2, N, L), dtype=np.int64)
    rot = np.zeros(N, dtype=np.uint64)
    d = np.zeros(L, dtype=np.int64)
    for p in range(2):
        poly = np.ascontiguousarray(acc[p * N:(p + 1) * N])
        lib.ora_monomial_mul(oracle.P(rot), oracle.P(poly), a_t, N)
        with np.errstate(over="ignore"):
            ct1 = rot - poly
        for j in range(N):
            lib.ora_decompose(int(ct1[j]), L, logB, d.ctypes.data_as(C.POINTER(C.c_int64)))
            out[p, j] = d
    return out


class Case:
    """One base: key, the nine ciphertexts (row 0 set by hand), two accumulators and the oracle's
    integer-mode outputs, computed once and shared by the batches (a ciphertext's output does not
    depend on the batch it runs in)."""

    def __init__(self, B, oracle, torch, logB):  # noqa: F811
        self.p = replace(B.CFG2, n=12, level=L, base_log=logB)
        self.S = Setup(B, oracle, torch, self.p, 8600 + logB)
        rng = np.random.RandomState(860 + logB)
        cts = encrypt(B, self.S, rng.randint(0, 4, size=NB), 2, 8650 + logB, std=2.0 ** -25)
        w = lambda t: np.uint64(t << 53)  # noqa: E731  (modulus switch: (x + 2^52) >> 53)
        edge = [w(1), np.uint64(0), np.uint64(5), w(2 * N - 1), w(N), w(1), w(2 * N - 1) + np.uint64(3),
                np.uint64((1 << 64) - 1)]  # the last rounds up to 2N = 0
        cts[0, :len(edge)] = edge
        cts[0, self.p.n] = np.uint64(7)  # body -> 0
        self.mask_ms = [oracle.lib().ora_modswitch(int(x), N) for x in cts[0]]
        self.cts = cts
        self.crafted = crafted_acc(logB, rng)
        self.accs = np.stack([self.crafted, lut_acc(B, self.S, rng.randint(0, 4, size=4), 2)])
        self.lut_idx = np.array([0, 1, 1, 0, 1, 1, 0, 1, 1], dtype=np.uint64)
        self.ref, _ = oracle.pbs_batch(self.S.op, cts, self.accs, bsk=self.S.bsk, lut_idx=self.lut_idx,
                                       mode=oracle.MODE_KARATSUBA)


_cases = {}


@pytest.fixture
def case(request, B, oracle, torch_cuda):  # noqa: F811
    logB = request.param
    if logB not in _cases:
        _cases[logB] = Case(B, oracle, torch_cuda, logB)
    return _cases[logB]


@pytest.mark.parametrize("case", BASES, indirect=True)
def test_crafted_row_reaches_edges_and_ties(oracle, case):
    """The hand-set row does what the other tests rely on (CPU only, the oracle's own functions):
    rotations by 1, 0, 2N - 1 and N with the body at 0, and in the first step's ct1 both tie cases
    at levels 0 and 1 and +B/2 at the last level, in both polynomials."""
    ms = case.mask_ms
    assert ms[case.p.n] == 0 and ms[0] == 1
    assert {0, 1, 2 * N - 1, N} <= set(ms[:case.p.n]) and case.cts[0, 1] == 0 and case.cts[0, 2] != 0 and ms[7] == 0
    half = 1 << (case.p.base_log - 1)
    dig = first_step_digits(oracle, case.crafted, case.p.base_log, ms[0])
    for p in range(2):
        for q in range(L - 1):
            assert (dig[p, :, q] == half).sum() >= 4, (p, q)    # field B/2, tie bit clear
            assert (dig[p, :, q] == -half).sum() >= 4, (p, q)   # field B/2, tie bit set
        assert (dig[p, :, L - 1] == half).sum() >= 4, p
        assert (dig[p, :, L - 1] == -half).sum() == 0, p        # nothing above the last level


@pytest.mark.parametrize("nb", BATCHES)
@pytest.mark.parametrize("case", BASES, indirect=True)
def test_slot_base_bit_exact(B, torch_cuda, monkeypatch, case, nb):  # noqa: F811
    """Batches 1, 4, 5, 9 (1, 5, 9: a last workgroup with one live ciphertext, whose idle waves run
    every barrier; 9: three workgroups) at bases 7 (fixed at compile time), 6 and 5 (read at run
    time): every output word equals the oracle's integer PBS."""
    monkeypatch.setenv("CONCRETE_HIP_PBS_SLOT", "1")
    got = run_gpu(B, case.S, case.cts[:nb], case.accs, torch_cuda, lut_idx=case.lut_idx[:nb])
    assert B.device_status("cuda:0") == 0
    assert np.array_equal(got, case.ref[:nb])


@pytest.mark.parametrize("case", [7], indirect=True)
def test_slot_base_resid_build(B, oracle, torch_cuda, monkeypatch, case):  # noqa: F811
    """The residual build of the fixed-base instance (it forms the rounded product explicitly and
    shares limb 2's rounding constant): bit-exact, measured residual below the certified bound."""
    monkeypatch.setenv("CONCRETE_HIP_PBS_SLOT", "1")
    got, r = run_gpu(B, case.S, case.cts, case.accs, torch_cuda, lut_idx=case.lut_idx, resid=True)
    assert B.device_status("cuda:0") == 0
    assert np.array_equal(got, case.ref)
    assert 0.0 < r < oracle.fft_error_bound(case.S.op, case.S.fbsk_cpu) < 0.5
