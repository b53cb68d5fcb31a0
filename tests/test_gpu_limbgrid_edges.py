"""Modulus-switch edge masks through every kernel of the 16-bit limb-grid family
(concrete_amd/csrc/pbs2048.hip, pbs1024k2.hip, pbs_small.hip, pbs512k4.hip).

The initial accumulator, the rotation ct1 = X^{at} acc - acc with its decomposer state, and the
recombination are one piece of code for the six kernels (kernel_util.hpp).  The fixed words of the
files' own test_edge_inputs were chosen for N = 1024; here the mask words sit on the boundaries of
each ring's own modulus switch.  The counterpart of test_gpu_pbs.py's
test_pbs_edge_masks_every_kernel.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (k, N, level, logB), one per kernel instantiation; (level, logB) are rows of test_gpu_pbs2048.py
# (CFG4, LEVEL_ROWS), test_gpu_pbs1024k2.py (opt4, test_tiny_n, K2_MANY_ROWS) and
# test_gpu_pbs_small.py (SHAPES / test_digit_forms, SM_LEVEL_ROWS, K4_LEVEL_ROWS, K4_MANY_ROWS)
CASES = [
    # pbs2048_quad_kernel<NQ = 1 .. 4>
    (1, 2048, 1, 23), (1, 2048, 2, 15), (1, 2048, 3, 11), (1, 2048, 4, 9),
    # pbs1024k2_kernel<NQ = 1, 2>, pbs1024k2_many_kernel at l = 3 and l = 5
    (2, 1024, 1, 23), (2, 1024, 2, 15), (2, 1024, 3, 12), (2, 1024, 5, 8),
    # pbs_small_kernel: two sub-digits, one, and the level rows
    (3, 512, 1, 18), (3, 512, 1, 15), (5, 256, 1, 18), (5, 256, 1, 15), (6, 256, 1, 18), (6, 256, 1, 15),
    (5, 256, 2, 10), (6, 256, 2, 12), (6, 256, 3, 9), (3, 512, 2, 12), (3, 512, 3, 9),
    # pbs512k4_kernel: two sub-digits, one, l = 2 on 13-bit limbs; pbs512k4_many_kernel at l = 3 and l = 6
    (4, 512, 1, 23), (4, 512, 1, 15), (4, 512, 2, 16), (4, 512, 3, 12), (4, 512, 6, 7),
]


def edge_words(N):
    """The six mask words on the boundaries of the switch to 2N: rotation by 0 (the skip rule); just
    below the rounding boundary (rounds to 0); the boundary (rounds up to 1: an odd rotation, the
    cross-parity path at N = 2048); rotation by N; 2N - 1 (odd, negated wrap); the largest word (rounds
    up to 2N = 0)."""
    s = 64 - (2 * N).bit_length() + 1  # 64 - log2(2N)
    return np.array([0, (1 << (s - 1)) - 1, 1 << (s - 1), 1 << 63, (2 * N - 1) << s, (1 << 64) - 1], dtype=np.uint64)


@pytest.mark.parametrize("k,N,level,logB", CASES, ids=lambda v: str(v))
def test_limbgrid_edge_masks_every_kernel(oracle, k, N, level, logB):
    """n = 6 and nine ciphertexts (a partly filled workgroup at 2 and at 4 ciphertexts per
    workgroup): six carry one edge word each in every mask position, three the six words rolled along
    the mask; random bodies, a random accumulator per ciphertext through lut_idx; bit for bit the
    exact oracle's result."""
    import torch

    from concrete_amd import backend as B
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    dev = "cuda:0"
    n, nb = 6, 9
    p = B.PbsParams(n=n, k=k, N=N, level=level, base_log=logB, ks_level=3, ks_base_log=4)
    assert B.pbs_supported(p)
    seed = 7000 + 97 * k + 13 * level + logB + N
    bsk = B.bsk_generate(p, B.binary_key(p.n, seed), B.binary_key(p.big_n, seed + 1), seed + 2)
    fbsk = B.convert_bsk(p, bsk, dev)
    words = edge_words(N)
    s = 64 - (2 * N).bit_length() + 1
    assert [((int(x) + (1 << (s - 1))) >> s) % (2 * N) for x in words] == [0, 0, 1, N, 2 * N - 1, 0]
    rng = np.random.RandomState(seed)

    def rand_u64(shape):
        return rng.randint(0, 1 << 32, size=shape).astype(np.uint64) << np.uint64(32) | \
            rng.randint(0, 1 << 32, size=shape).astype(np.uint64)

    cts = rand_u64((nb, n + 1))
    for j in range(6):
        cts[j, :n] = words[j]
    for j in range(3):
        cts[6 + j, :n] = np.roll(words, j)
    accs = rand_u64((nb, (k + 1) * N))
    lut_idx = rng.permutation(nb).astype(np.uint64)
    out = torch.zeros((nb, p.lwe_out_size), dtype=torch.int64, device=dev)
    B.pbs(p, fbsk, B.to_device(cts, dev), B.to_device(accs, dev), out=out, num_samples=nb,
          lut_idx=B.to_device(lut_idx, dev))
    torch.cuda.synchronize()
    assert B.device_status(dev) == 0
    op = oracle.Params(n=n, k=k, N=N, l=level, logB=logB)
    ref, _ = oracle.pbs_batch(op, cts, accs, bsk=bsk, mode=oracle.MODE_KARATSUBA, lut_idx=lut_idx)
    assert np.array_equal(B.to_host(out), ref)
