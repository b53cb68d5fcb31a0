"""GPU sweep over the optimizer's two 128-bit tables (tests/table_shapes.py): every distinct PBS
shape (k, N, br_l, br_b) and every distinct keyswitch decomposition (ks_l, ks_b) is launched once and compared
word for word with the oracle's integer arithmetic (oracle.pbs_batch in Karatsuba mode,
oracle.keyswitch_batch).  There is no tolerance anywhere.

Collection stays free of the native library: the parameter lists and ids below come from table_shapes and
literals only.  Key format, dispatch class and bounds are computed inside the test bodies, after the `env`
fixture has imported torch (a process that loads libconcrete_hip.so before torch maps two HIP runtimes,
DESIGN.md §5; tests/test_keygen_abi.py::test_table_sweeps_are_complete_and_collect_without_the_library pins
both the lists and the import order).

A shape leaves a sweep only through NOT_SWEPT, with its evidence; that CPU test asserts that swept and
not-swept shapes together are the table's list.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_shapes as S  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A

# {(k, N, br_l, br_b): reason} for PBS shapes, {(ks_l, ks_b): reason} for keyswitch decompositions
NOT_SWEPT = {}
KS_NOT_SWEPT = {}

PBS_SWEPT = [s for s in S.PBS_SHAPES if s not in NOT_SWEPT]
KS_SWEPT = [d for d in S.KS_DECOMPS if d not in KS_NOT_SWEPT]


def pbs_steps(N):
    """CMUX steps of a swept shape: as many as keep the oracle's O(N^1.6) product inside a few seconds, never
    fewer than 2, so that the second step decomposes the non-trivial mask the first one produced."""
    return 4 if N <= 8192 else 3 if N == 16384 else 2


def _widths():
    w = {}
    for r in S.V0_ROWS:
        s = tuple(r[c] for c in S.PBS_COLS)
        w[s] = min(w.get(s, 64), r["bits"])
    return w


# message width of a shape: the narrowest v0 row that has it; 3 for the shapes only the WoP table has
WIDTH = _widths()


def pbs_width(shape):
    return WIDTH.get(shape, 3)


def pbs_id(s):
    return "k%dN%dl%db%d" % s


def ks_id(d):
    return "l%db%d" % d


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from concrete_amd import _native
    from concrete_amd import backend as B
    from oracle import pyoracle as O
    O.lib()
    return dict(torch=torch, L=_native.lib(), B=B, O=O, ksk={})


def _rand_u64(rng, shape):
    return rng.randint(0, 1 << 32, size=shape).astype(np.uint64) << np.uint64(32) | \
        rng.randint(0, 1 << 32, size=shape).astype(np.uint64)


def _filled(env, shape):
    t = env["torch"].empty(shape, dtype=env["torch"].int64, device=DEV)
    t.fill_(SENTINEL)  # below 2^63: the same bits as int64
    return t


def error_bound(B, O, p, op, bsk, fbsk):
    """The certified rounding bound of the key's kind, as test_generic_pbs_bit_exact chooses it; kind 1 (the
    N = 1024, k = 1 kernels; no table shape today) as tests/test_gpu_pbs.py does."""
    kind, limbs, bits = B.bsk_format(p)
    if kind == 1:
        return O.fft_error_bound(op, O.bsk_to_fourier(op, bsk))
    key = B.to_host(fbsk).view(np.float64)
    if kind == 2:
        return O.gpu2048_error_bound(key, p.base_log, p.level)
    if kind == 4:
        return O.gpu1024k2_error_bound(key, p.base_log, p.level)
    if kind == 5:
        return O.gpu_small_error_bound(key, p.N, p.k, p.base_log, p.level)
    assert kind == 3, kind
    return O.generic_error_bound(p.k, p.N, p.level, p.base_log, bits, key)


# ---------------------------------------------------------------------------------------------------------
# A. PBS: every (k, N, br_l, br_b) of both tables
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PBS_SWEPT, ids=pbs_id)
def test_pbs_table_shape_bit_exact(env, shape):
    """5 ciphertexts at n = pbs_steps(N), permuted input and output rows, and two accumulators: the trivial GLWE
    of a random table, and a GLWE of uniformly random words in mask and body (the ABI takes any GLWE; its mask
    rows meet full-magnitude digits from the first step on)."""
    B, O, torch = env["B"], env["O"], env["torch"]
    k, N, level, base_log = shape
    width = pbs_width(shape)
    seed = 880000 + 100 * S.PBS_SHAPES.index(shape)
    p = B.PbsParams(n=pbs_steps(N), k=k, N=N, level=level, base_log=base_log)
    assert B.pbs_supported(p), p
    lwe_sk, glwe_sk = B.binary_key(p.n, seed), B.binary_key(p.big_n, seed + 1)
    bsk = B.bsk_generate(p, lwe_sk, glwe_sk, seed + 2)
    fbsk = B.convert_bsk(p, bsk, DEV)
    rng = np.random.RandomState(seed % (1 << 31))
    table = rng.randint(0, 1 << width, size=1 << width).astype(np.uint64)
    msgs = rng.randint(0, 1 << width, size=5)
    # n is far below a secure LWE dimension, so the inputs carry a small fixed noise (test_gpu_pbs_generic.py)
    cts = B.lwe_encrypt(lwe_sk, [B.encode(m, width) for m in msgs], p.n, 2.0 ** -30, seed + 3)
    luts = np.stack([B.trivial_glwe(p, B.expand_lut(table, p.N, width)), _rand_u64(rng, p.glwe_size)])
    in_idx = np.array([3, 0, 4, 1, 2], dtype=np.uint64)
    out_idx = np.array([1, 4, 0, 2, 3], dtype=np.uint64)
    lut_idx = np.array([0, 1, 0, 1, 0], dtype=np.uint64)
    d = {name: B.to_device(a, DEV) for name, a in (("in_idx", in_idx), ("out_idx", out_idx), ("lut_idx", lut_idx))}
    out = _filled(env, (6, p.lwe_out_size))  # one row more than the call writes
    resid = torch.zeros(1, dtype=torch.int64, device=DEV)
    B.pbs(p, fbsk, B.to_device(cts, DEV), B.to_device(luts, DEV), out=out, num_samples=5, resid=resid, **d)
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got = B.to_host(out)
    op = O.Params(n=p.n, k=p.k, N=p.N, l=p.level, logB=p.base_log)
    ref, _ = O.pbs_batch(op, cts, luts, bsk=bsk, mode=O.MODE_KARATSUBA, lut_idx=lut_idx, in_idx=in_idx,
                         out_idx=out_idx)
    assert ref.shape == (5, p.lwe_out_size)
    bad = np.nonzero((got[:5] != ref).any(axis=1))[0]
    assert bad.size == 0, f"{pbs_id(shape)}: output rows {bad.tolist()} differ from the exact oracle"
    assert (got[5] == np.uint64(SENTINEL)).all(), "wrote past the output"
    seen = float(B.to_host(resid).view(np.float64)[0])
    bound = error_bound(B, O, p, op, bsk, fbsk)
    print(f"{pbs_id(shape)}: format {B.bsk_format(p)}, residual {seen:.3e}, bound {bound:.3e}")
    assert seen < bound < 0.5, (seen, bound)
    dec = B.lwe_decrypt(glwe_sk, got[:5], p.big_n)
    plain = [s for s in range(5) if lut_idx[s] == 0]
    assert [B.decode(dec[int(out_idx[s])], width) for s in plain] == [int(table[msgs[int(in_idx[s])]]) for s in plain]


# ---------------------------------------------------------------------------------------------------------
# B. keyswitch: every (ks_l, ks_b) of both tables, on the VALU kernel and on the matrix-core kernel
# ---------------------------------------------------------------------------------------------------------
KS_N_IN, KS_N_OUT = 200, 600  # K = 200 l bytes of digits a row: whole 64-byte blocks only when 8 divides l;
#                               601 output words: neither a multiple of the 64-column tile nor of 256 threads
KS_BATCHES = (5, 67)          # below / from KS_MFMA_MIN_BATCH = 64 (keyswitch.hip): the VALU / the matrix-core kernel


def ks_valu_chunks(level, base_log):
    """keyswitch.hip:keyswitch_launch: the VALU kernel's int32 chunk form by the largest digit row sum
    l 2^(base_log-1): 3 chunks up to 32, 4 chunks up to 1024, else (0) the 64-bit products."""
    dmax = level << (base_log - 1)
    return 3 if dmax <= 32 else 4 if dmax <= 1024 else 0


# over the 29 decompositions: (3, 5), (5, 4) and (6, 4) take 4 chunks (row sums 48, 40, 48), the other 26 take 3
KS_FOUR_CHUNKS = [(3, 5), (5, 4), (6, 4)]


def _ks_case(env, decomp):
    """A real key (concrete_hip_ksk_generate) 200 -> 600 and 67 rows of random odd words, once per decomposition."""
    if decomp in env["ksk"]:
        return env["ksk"][decomp]
    B, O = env["B"], env["O"]
    level, base_log = decomp
    seed = 890000 + 100 * S.KS_DECOMPS.index(decomp)
    p = B.PbsParams(n=KS_N_OUT, k=1, N=KS_N_IN, level=1, base_log=1, ks_level=level, ks_base_log=base_log)
    ksk = B.ksk_generate(p, B.binary_key(KS_N_IN, seed), B.binary_key(KS_N_OUT, seed + 1), seed + 2)
    rng = np.random.RandomState(seed)
    cts = rng.randint(0, 2 ** 63, size=(max(KS_BATCHES), KS_N_IN + 1), dtype=np.int64).astype(np.uint64) * \
        np.uint64(2) + np.uint64(1)
    op = O.Params(n=KS_N_OUT, k=1, N=KS_N_IN, l=1, logB=1, ks_l=level, ks_logB=base_log)
    want = O.keyswitch_batch(op, cts, ksk)
    for a in (cts, want):
        a.setflags(write=False)
    c = dict(p=p, cts=cts, want=want, d_ksk=B.to_device(ksk, DEV))
    env["ksk"] = {decomp: c}  # one key on the device at a time
    return c


@pytest.mark.parametrize("case", [(d, b) for d in KS_SWEPT for b in KS_BATCHES], ids=lambda c: f"{ks_id(c[0])}-b{c[1]}")
def test_keyswitch_table_decomposition_bit_exact(env, case):
    B, torch = env["B"], env["torch"]
    (level, base_log), batch = case
    assert env["L"].concrete_hip_keyswitch_supported(level, base_log, KS_N_IN, KS_N_OUT) == 1
    # every table decomposition is exact on the matrix cores (keyswitch.hip:ks_mfma_ok) and has an int32 chunk form
    assert base_log <= 7 and KS_N_IN * level * (1 << (base_log - 1)) * 128 <= 0x7FFFFFFF
    assert ks_valu_chunks(level, base_log) == (4 if (level, base_log) in KS_FOUR_CHUNKS else 3)
    c = _ks_case(env, (level, base_log))
    out = _filled(env, (batch + 1, KS_N_OUT + 1))  # one row more than the call writes
    B.keyswitch(c["p"], c["d_ksk"], B.to_device(c["cts"][:batch].copy(), DEV), out=out, num_samples=batch)
    torch.cuda.synchronize()
    got = B.to_host(out)
    assert np.array_equal(got[:batch], c["want"][:batch]), f"{ks_id(case[0])}, batch {batch}: differs from the oracle"
    assert (got[batch] == np.uint64(SENTINEL)).all(), "wrote past the output"
