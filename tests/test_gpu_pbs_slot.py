"""GPU tests of the slot-split cfg2 kernel (pbs1024_pair_slot_kernel, concrete_amd/csrc/pbs.hip):
four ciphertexts per workgroup, each of the eight waves taking one frequency slot of the key
products for all of them, the key in registers.  CONCRETE_HIP_PBS_SLOT=1 forces it for a whole call,
=0 keeps the ring kernel in the planned call; everything is bit-exact against the CPU oracle.
"""
from dataclasses import replace

import numpy as np
import pytest

from test_gpu_pbs import B, Setup, cfg2, encrypt, lut_acc, run_gpu, run_oracle, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,base_log,nb", [(1, 3, 1), (1, 7, 5), (2, 9, 4), (3, 1, 9), (12, 7, 13), (12, 3, 9),
                                           (12, 9, 3), (2, 1, 13), (3, 7, 1), (1, 9, 4), (12, 1, 5), (3, 3, 3)])
def test_pbs_slot_kernel(B, oracle, torch_cuda, monkeypatch, n, base_log, nb):  # noqa: F811
    """The kernel forced on small shapes: blind rotations of 1-12 steps (the key prefetch's prologue
    and the last step's re-read), the edges of the exact range's logB, ragged batches (nb = 1 leaves
    seven waves doing slot work only; nb = 5, 9, 13 end in a workgroup with one live ciphertext),
    permuted index arrays and per-sample LUTs; bit-exact vs the oracle with the measured rounding
    residual below the certified bound."""
    monkeypatch.setenv("CONCRETE_HIP_PBS_SLOT", "1")
    p = replace(B.CFG2, n=n, level=3, base_log=base_log)
    S = Setup(B, oracle, torch_cuda, p, 7400 + 10 * n + base_log)
    width = 2
    rng = np.random.RandomState(nb * 100 + n)
    tables = [rng.randint(0, 4, size=4) for _ in range(nb)]
    msgs = rng.randint(0, 4, size=nb)
    cts = encrypt(B, S, msgs, width, 81 + n, std=2.0 ** -25)
    accs = np.stack([lut_acc(B, S, t, width) for t in tables])
    in_idx = rng.permutation(nb).astype(np.uint64)
    out_idx = rng.permutation(nb).astype(np.uint64)
    lut_idx = rng.permutation(nb).astype(np.uint64)
    dev = "cuda:0"
    resid = torch_cuda.zeros(1, dtype=torch_cuda.int64, device=dev)
    out = B.pbs(p, S.fbsk, B.to_device(cts, dev), B.to_device(accs, dev), lut_idx=B.to_device(lut_idx, dev),
                in_idx=B.to_device(in_idx, dev), out_idx=B.to_device(out_idx, dev), resid=resid)
    torch_cuda.cuda.synchronize()
    assert B.device_status(dev) == 0
    got = B.to_host(out)
    ref, _ = oracle.pbs_batch(S.op, cts[in_idx.astype(np.int64)], accs, fbsk=S.fbsk_cpu, lut_idx=lut_idx)
    exp = np.zeros_like(ref)
    exp[out_idx.astype(np.int64)] = ref
    assert np.array_equal(got, exp)
    r = float(np.array([int(resid.cpu()[0])], dtype=np.int64).view(np.float64)[0])
    assert r < oracle.fft_error_bound(S.op, S.fbsk_cpu) < 0.5


def test_pbs_slot_kernel_cfg2_full(B, oracle, cfg2, torch_cuda, monkeypatch):  # noqa: F811
    """The full cfg2 row (n = 630): 67 ciphertexts bit-exact vs the oracle, every one decrypting to
    its LUT entry, residual under the bound."""
    monkeypatch.setenv("CONCRETE_HIP_PBS_SLOT", "1")
    width = 3
    rng = np.random.RandomState(73)
    table = rng.randint(0, 8, size=8)
    msgs = rng.randint(0, 8, size=67)
    cts = encrypt(B, cfg2, msgs, width, 83)
    acc = lut_acc(B, cfg2, table, width)
    got, resid = run_gpu(B, cfg2, cts, acc, torch_cuda, resid=True)
    ref = run_oracle(oracle, cfg2, cts, acc)
    assert np.array_equal(got, ref)
    assert resid < oracle.fft_error_bound(cfg2.op, cfg2.fbsk_cpu) < 0.5
    dec = B.lwe_decrypt(cfg2.glwe_sk, got, cfg2.p.big_n)
    assert [B.decode(d, width) for d in dec] == [int(table[m]) for m in msgs]


class Planned:
    """One planned batch (whole pair rounds only: 4 x CUs - 9 ciphertexts, n = 12) and its oracle
    outputs, shared by the tests below."""

    def __init__(self, B, oracle, torch):  # noqa: F811
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.nb = nb = 4 * cus - 9
        self.p = replace(B.CFG2, n=12)
        self.S = Setup(B, oracle, torch, self.p, 7900)
        rng = np.random.RandomState(nb)
        cts = encrypt(B, self.S, rng.randint(0, 4, size=nb), 2, 7901, std=2.0 ** -25)
        accs = np.stack([lut_acc(B, self.S, rng.randint(0, 4, size=4), 2) for _ in range(3)])
        lut_idx = rng.randint(0, 3, size=nb).astype(np.uint64)
        self.ref, _ = oracle.pbs_batch(self.S.op, cts, accs, fbsk=self.S.fbsk_cpu, lut_idx=lut_idx)
        self.d_in, self.d_acc = B.to_device(cts, "cuda:0"), B.to_device(accs, "cuda:0")
        self.d_lut_idx = B.to_device(lut_idx, "cuda:0")

    def run(self, B, torch):  # noqa: F811
        out = B.to_host(B.pbs(self.p, self.S.fbsk, self.d_in, self.d_acc, lut_idx=self.d_lut_idx))
        torch.cuda.synchronize()
        assert B.device_status("cuda:0") == 0
        return out


@pytest.fixture(scope="module")
def planned(B, oracle, torch_cuda):  # noqa: F811
    return Planned(B, oracle, torch_cuda)


def test_pbs_slot_equals_ring_kernel(B, planned, torch_cuda, monkeypatch):  # noqa: F811
    """Old equals new: the same inputs through the ring kernel (CONCRETE_HIP_PBS_PAIRS=4) and through
    the slot-split kernel give equal outputs."""
    monkeypatch.setenv("CONCRETE_HIP_PBS_PAIRS", "4")
    old = planned.run(B, torch_cuda)
    monkeypatch.delenv("CONCRETE_HIP_PBS_PAIRS")
    monkeypatch.setenv("CONCRETE_HIP_PBS_SLOT", "1")
    new = planned.run(B, torch_cuda)
    assert np.array_equal(old, new)
    assert np.array_equal(new, planned.ref)


def test_pbs_slot_fallback(B, planned, torch_cuda, monkeypatch):  # noqa: F811
    """CONCRETE_HIP_PBS_SLOT=0 keeps the ring kernel in a planned call: bit-exact, as is the default."""
    from concrete_amd import _native
    import ctypes as C
    parts = (C.c_uint32 * 3)()
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    _native.lib().concrete_hip_pbs1024_plan(planned.nb, cus, parts)
    assert parts[0] > 0, list(parts)  # the plan has a pair part
    monkeypatch.setenv("CONCRETE_HIP_PBS_SLOT", "0")
    assert np.array_equal(planned.run(B, torch_cuda), planned.ref)
    monkeypatch.delenv("CONCRETE_HIP_PBS_SLOT")
    assert np.array_equal(planned.run(B, torch_cuda), planned.ref)
