"""GPU tests of the slot-split cfg2 kernel's step schedule (pbs1024_pair_slot_kernel,
concrete_amd/csrc/pbs.hip): the inverse's last twiddle fused into the rounding,
transforms interleaved with each other and with product windows.  The kernel is forced with
CONCRETE_HIP_PBS_SLOT=1; everything is bit-exact against the CPU oracle.
"""
from dataclasses import replace

import numpy as np
import pytest

from test_gpu_pbs import B, Setup, encrypt, lut_acc, run_gpu, run_oracle, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


def check(B, oracle, torch, S, cts, accs, lut_idx=None, resid=True):  # noqa: F811
    """The plain kernel (the one a PBS call runs: its rounding is the fused FMA) always; with resid
    also the residual build of the same inputs (it forms the rounded product explicitly, so it is
    another instantiation of the kernel), both bit-exact against one oracle run."""
    ref = run_oracle(oracle, S, cts, accs, lut_idx=lut_idx)
    got = run_gpu(B, S, cts, accs, torch, lut_idx=lut_idx, resid=False)
    assert B.device_status("cuda:0") == 0
    assert np.array_equal(got, ref)
    if resid:
        got, r = run_gpu(B, S, cts, accs, torch, lut_idx=lut_idx, resid=True)
        assert B.device_status("cuda:0") == 0
        assert np.array_equal(got, ref)
        assert r < oracle.fft_error_bound(S.op, S.fbsk_cpu) < 0.5


# n in {1, 2, 3}: the pipeline's prologue and the last step's re-read; logB in {1, 7, 9} x
# nb in {1, 4, 7}: the edges of the exact range and workgroups with 1, 4 and 3 live ciphertexts;
# n = 40, nb = 6: 200 exchanges (every reuse of a mailbox and of the published scratch runs many
# times), the second workgroup with two live ciphertexts
@pytest.mark.parametrize("n,base_log,nb", [(1, 1, 1), (2, 1, 4), (3, 1, 7), (2, 7, 1), (3, 7, 4), (1, 7, 7),
                                           (3, 9, 1), (1, 9, 4), (2, 9, 7), (40, 7, 6)])
def test_slot_sched_ragged_workgroups(B, oracle, torch_cuda, monkeypatch, n, base_log, nb):  # noqa: F811
    monkeypatch.setenv("CONCRETE_HIP_PBS_SLOT", "1")
    p = replace(B.CFG2, n=n, level=3, base_log=base_log)
    S = Setup(B, oracle, torch_cuda, p, 8100 + 10 * n + base_log)
    rng = np.random.RandomState(1000 * n + 10 * base_log + nb)
    cts = encrypt(B, S, rng.randint(0, 4, size=nb), 2, 8101 + n, std=2.0 ** -25)
    accs = np.stack([lut_acc(B, S, rng.randint(0, 4, size=4), 2) for _ in range(nb)])
    check(B, oracle, torch_cuda, S, cts, accs, lut_idx=rng.permutation(nb).astype(np.uint64))


def test_slot_sched_edge_masks(B, oracle, torch_cuda, monkeypatch):  # noqa: F811
    """Mask words set by hand: 0 (rotation by 0, the skip rule), 2^53 - 1 (just below a modulus-switch
    rounding boundary), 2^63 (rotation by N) and 2^64 - 1 (the largest round-up, to 2N = 0); one
    value per ciphertext in the first workgroup, all four mixed per step in the second."""
    monkeypatch.setenv("CONCRETE_HIP_PBS_SLOT", "1")
    p = replace(B.CFG2, n=4, level=3, base_log=7)
    S = Setup(B, oracle, torch_cuda, p, 8200)
    rng = np.random.RandomState(82)
    cts = encrypt(B, S, rng.randint(0, 4, size=8), 2, 8201, std=2.0 ** -25)
    words = np.array([0, (1 << 53) - 1, 1 << 63, (1 << 64) - 1], dtype=np.uint64)
    for j in range(4):
        cts[j, : p.n] = words[j]
        cts[4 + j, : p.n] = np.roll(words, j)
    accs = np.stack([lut_acc(B, S, rng.randint(0, 4, size=4), 2) for _ in range(8)])
    check(B, oracle, torch_cuda, S, cts, accs, lut_idx=np.arange(8, dtype=np.uint64), resid=False)


def test_slot_sched_large_digits(B, oracle, torch_cuda, monkeypatch):  # noqa: F811
    """LUT coefficients uniform over the whole u64 range at logB = 9: decomposition digits of every
    size (up to 2^8 in magnitude) and full-range products reach the fused last twiddle and rounding
    (the plain kernel's single FMA, and the residual build's explicit product)."""
    monkeypatch.setenv("CONCRETE_HIP_PBS_SLOT", "1")
    p = replace(B.CFG2, n=12, level=3, base_log=9)
    S = Setup(B, oracle, torch_cuda, p, 8300)
    rng = np.random.RandomState(83)
    nb = 12
    cts = encrypt(B, S, rng.randint(0, 4, size=nb), 2, 8301, std=2.0 ** -25)
    luts = rng.randint(0, 1 << 32, size=(nb, p.N)).astype(np.uint64) << np.uint64(32)
    luts |= rng.randint(0, 1 << 32, size=(nb, p.N)).astype(np.uint64)
    accs = np.stack([B.trivial_glwe(p, lut) for lut in luts])
    check(B, oracle, torch_cuda, S, cts, accs, lut_idx=np.arange(nb, dtype=np.uint64))
