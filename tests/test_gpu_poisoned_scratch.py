"""Every path that reads scratch memory, run on poisoned scratch and held to the exact words.

The library's working memory is stream-ordered pool memory that stays mapped between calls
(concrete_amd/csrc/abi.hip keep_pool_memory), and callers may hand in scratch of their own: a call starts on
whatever an earlier call left there.  A kernel that reads a scratch word before any kernel wrote it sees zeros in
a fresh process, plausible numbers after a test of a similar shape, and anything in a long-running runtime.  The
test hook CONCRETE_HIP_SCRATCH_FILL (abi.hip pool_alloc / scratch_fill) sets every scratch allocation of the
library to one byte before the call's kernels run; the caller-provided buffers are filled here.  Two bytes:

    0xFF   u64: all ones; f64: a NaN; int8: -1; a u32 flag: above any event count
    0x7F   f64: 1.4e306, two of them sum to infinity; int8: 127

Every case, under both: the output equals the exact reference word for word, it equals the same call's output
with the hook unset, and a reported rounding residual is bit-identical to the clean run's and below the certified
bound.  The expected words and the clean run are made once per case (REF, CLEAN) and shared by the fills.
test_the_knob_is_live proves that the fills reach the memory; without it the rest could pass vacuously.

Layouts poisoned: the general path's X / Y / accumulator scratch of the two-launch, four-step and split paths
(whole and in chunks on two streams), the N = 8192 hand-off buffers and flags, the key conversions' staging,
tables and spectrum sink, the split conversion's scratch, the keyswitch's int8 digit matrix and key bytes (pool
and cached branch), the WoP stages' carve-outs of a caller's buffer and of the scratch_cuda_* buffers, the
runtime's and the stream emulator's slice staging buffers.  The general path's tile kernels and the fused
N = 4096 kernel keep their state in LDS and registers and take no scratch: they have no case here.
"""
import ctypes as C
import os
import sys
from dataclasses import replace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_circuit_bootstrap as TC  # noqa: E402
import test_gpu_extract_bits as TE  # noqa: E402
import test_gpu_pbs_generic as TG  # noqa: E402
import test_gpu_sdfg_graph as TS  # noqa: E402
import test_gpu_vertical_packing as TV  # noqa: E402
import vp_reference as V  # noqa: E402
import wop_cases as Cs  # noqa: E402
import wop_reference as W  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KNOB = "CONCRETE_HIP_SCRATCH_FILL"
FILLS = (0xFF, 0x7F)
FILL_IDS = ["ff", "7f"]
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD_BYTE, GUARD_BYTES = 0x5A, 32768
REF = {}    # case -> the exact reference's words (and what else the case's checks need), made once
CLEAN = {}  # case -> the call's result with the hook unset, made once


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from concrete_amd import _native
    from concrete_amd import backend as B
    from concrete_amd import runtime as RT
    from oracle import pyoracle as O
    O.lib()
    e = dict(torch=torch, L=_native.lib(), B=B, O=O, N=_native, RT=RT)
    # what the other GPU files' case builders expect of their `env`: the dictionaries they keep keys and cases in
    e.update(te=dict(e, setups={}), tc=dict(e, fpks={}, cbs={}, keys={}), tv=dict(e, keys={}, cases={}))
    return e


def both(monkeypatch, fill, case, run):
    """(the clean run's result, made once per case with the hook unset; the result of run(fill) under the fill)."""
    if case not in CLEAN:
        monkeypatch.delenv(KNOB, raising=False)
        CLEAN[case] = run(None)
    monkeypatch.setenv(KNOB, hex(fill))
    return CLEAN[case], run(fill)


def once(case, make):
    if case not in REF:
        REF[case] = make()
    return REF[case]


def resid_bits(t):
    return int(t.item())


def as_f64(bits):
    return float(np.array([bits], dtype=np.int64).view(np.float64)[0])


def filled(env, shape):
    t = env["torch"].empty(shape, dtype=env["torch"].int64, device=DEV)
    t.fill_(SENTINEL)
    return t


def callers_scratch(env, need, fill):
    """A caller's scratch of exactly `need` bytes, every byte `fill`, and the guard bytes right behind it; (None,
    None) for the clean run, which takes pool scratch."""
    torch = env["torch"]
    if fill is None:
        return None, None
    assert need > 0 and need % 16 == 0
    buf = torch.full((need + GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    buf[:need] = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
    scratch, guard = buf[:need], buf[need:]
    assert scratch.data_ptr() % 16 == 0 and scratch.numel() * scratch.element_size() == need
    return scratch, guard


def guard_intact(guard):
    return guard is None or bool((guard == GUARD_BYTE).all())


# ---------------------------------------------------------------------------------------------------------
# 2.0 the hook is live
# ---------------------------------------------------------------------------------------------------------
def test_the_knob_is_live(env, monkeypatch):
    """With the hook at 0xA5, a cuda_malloc_async buffer and a scratch_cuda_extract_bits_64 buffer read back as
    0xA5 in every byte."""
    L, B = env["L"], env["B"]
    monkeypatch.setenv(KNOB, "0xA5")
    s = L.cuda_create_stream(0)
    try:
        size = 3 * 4096 + 7
        d = L.cuda_malloc_async(size, s, 0)
        host = np.zeros(size, dtype=np.uint8)
        L.cuda_memcpy_async_to_cpu(host.ctypes.data, d, size, s, 0)
        L.cuda_synchronize_device(0)
        L.cuda_drop(d, 0)
        assert (host == 0xA5).all(), f"{int((host != 0xA5).sum())} of {size} bytes of cuda_malloc_async's buffer"
        p, rows = replace(B.CFG2, n=8), 3
        size = B.extract_bits_scratch_bytes(p, rows, 63)  # what the scratch call sizes the buffer for
        assert size > 0
        buf = C.c_void_p(None)
        L.scratch_cuda_extract_bits_64(s, 0, C.byref(buf), p.k, p.n, p.N, p.level, rows, 0, True)
        assert buf.value
        host = np.zeros(size, dtype=np.uint8)
        L.cuda_memcpy_async_to_cpu(host.ctypes.data, buf, size, s, 0)
        L.cuda_synchronize_device(0)
        L.cleanup_cuda_extract_bits(s, 0, C.byref(buf))
        assert (host == 0xA5).all(), f"{int((host != 0xA5).sum())} of {size} bytes of the extract-bits buffer"
    finally:
        L.cuda_synchronize_device(0)
        L.cuda_destroy_stream(s, 0)


# ---------------------------------------------------------------------------------------------------------
# 2.1 the general path
# ---------------------------------------------------------------------------------------------------------
GEN_CASES = {c[0]: c for c in TG.CASES}
# (id, label in test_gpu_pbs_generic.CASES, batch, environment of the call)
PBS_ROWS = [
    ("two_launch_N512", "k3_N512_l4", 5, {}),
    # three chunks on two streams, the last one of a single ciphertext
    ("two_launch_N512_chunks", "k3_N512_l4", 5, {"CONCRETE_HIP_GEN_CHUNK": "2"}),
    ("two_launch_N1024", "k3_N1024_l2", 5, {}),
    ("four_step_N2048", "k1_N2048_l5", 3, {}),
    ("four_step_N4096_wide_state", "k1_N4096_l3_wide_state", 3, {}),
    ("four_step_N16384", "8bit_k1_N16384", 2, {}),
    ("two_workgroups_N8192", "7bit_k1_N8192", 3, {}),
    # the X / Y hand-off buffers of a second chunk, the flags re-zeroed per chunk
    ("two_workgroups_N8192_chunks", "7bit_k1_N8192", 3, {"CONCRETE_HIP_GEN_CHUNK": "2"}),
    ("two_launch_N8192", "7bit_k1_N8192", 3, {"CONCRETE_HIP_GEN_COOP": "0"}),
    ("split_N32768", "9bit_k1_N32768", 2, {}),   # these two also convert the key on the split path
    ("split_N65536", "10bit_k1_N65536", 2, {}),
]


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("row", PBS_ROWS, ids=[r[0] for r in PBS_ROWS])
def test_general_path_pbs(env, monkeypatch, row, fill):
    """The key is converted under the fill too (staging, tables, the split conversion's scratch)."""
    B, O, torch = env["B"], env["O"], env["torch"]
    name, label, batch, extra = row
    case = GEN_CASES[label]
    for var, val in extra.items():
        monkeypatch.setenv(var, val)

    def clean():
        monkeypatch.delenv(KNOB, raising=False)
        p, glwe_sk, bsk, fbsk, cts, acc, table, msgs, got, resid = TG.run_case(B, O, torch, case, 9100, batch=batch)
        op = O.Params(n=p.n, k=p.k, N=p.N, l=p.level, logB=p.base_log)
        ref, _ = O.pbs_batch(op, cts, acc[None, :], bsk=bsk, mode=O.MODE_KARATSUBA)
        kind, limbs, bits = B.bsk_format(p)
        assert kind == 3, "a case of the general path"
        bound = O.generic_error_bound(p.k, p.N, p.level, p.base_log, bits, B.to_host(fbsk).view(np.float64))
        return dict(p=p, bsk=bsk, cts=cts, acc=acc, ref=ref, got=got, resid=resid, bound=bound)

    c = once(("pbs", name), clean)
    assert np.array_equal(c["got"], c["ref"]), "the clean run differs from the exact oracle"
    p = c["p"]
    monkeypatch.setenv(KNOB, hex(fill))
    fbsk = B.convert_bsk(p, c["bsk"], DEV)
    r = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = filled(env, (batch + 1, p.lwe_out_size))  # one row more than the call writes
    B.pbs(p, fbsk, B.to_device(c["cts"], DEV), B.to_device(c["acc"][None, :], DEV), out=out, num_samples=batch, resid=r)
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got, resid = B.to_host(out), as_f64(resid_bits(r))
    print(f"{name} fill {fill:#x}: residual {resid!r} (clean {c['resid']!r}), bound {c['bound']:.3e}")
    assert np.array_equal(got[:batch], c["ref"]), f"{int((got[:batch] != c['ref']).sum())} words differ from the oracle"
    assert np.array_equal(got[:batch], c["got"]), "differs from the clean run"
    assert (got[batch] == np.uint64(SENTINEL)).all(), "wrote past the output"
    assert resid == c["resid"], "the residual differs from the clean run's"
    assert resid < c["bound"] < 0.5


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_hand_tuned_ring_on_its_companion_key(env, monkeypatch, fill):
    """cfg2's ring at l = 1, logB = 23 (tests/test_gpu_runtime.py test_wide_digits_on_the_general_path): digits the
    pair kernel refuses, run on the general-format companion of the key, which a keyset builds from the standard
    key under the fill, and on a caller-converted general-format key with the residual reported; batch 3."""
    B, O, RT, L, torch = env["B"], env["O"], env["RT"], env["L"], env["torch"]
    p = replace(B.CFG2, n=12, level=1, base_log=23)
    batch, width = 3, 3

    def make():
        lwe_sk, glwe_sk = B.binary_key(p.n, 81), B.binary_key(p.big_n, 82)
        bsk = B.bsk_generate(p, lwe_sk, glwe_sk, 83, std=2.0 ** -52)
        table = np.array([4, 1, 6, 3, 0, 7, 2, 5], dtype=np.uint64)
        tlu = B.expand_lut(table, p.N, width)
        acc = B.trivial_glwe(p, tlu)
        cts = B.lwe_encrypt(lwe_sk, [B.encode(m, width) for m in (5, 0, 3)], p.n, 2.0 ** -25, 84)
        op = O.Params(n=p.n, k=p.k, N=p.N, l=p.level, logB=p.base_log)
        ref, _ = O.pbs_batch(op, cts, acc[None, :], bsk=bsk, mode=O.MODE_KARATSUBA)
        return dict(bsk=bsk, tlu=tlu, acc=acc, cts=cts, ref=ref)

    c = once("companion", make)
    assert L.concrete_hip_pbs_supported(p.k, p.N, p.level, p.base_log) == 1

    def run(_):
        ks = RT.Keyset([0])
        ks.add_bsk(0, c["bsk"], p)
        via_keyset = RT.batched_bootstrap(ks, p, c["cts"], c["tlu"])
        ks.close()
        g = torch.zeros(L.concrete_hip_generic_bsk_size_bytes(p.n, p.k, p.level, p.N) // 8, dtype=torch.int64, device=DEV)
        st = B._stream(DEV)
        env["N"].check(L.concrete_hip_convert_bsk_generic(st, 0, g.data_ptr(), c["bsk"].ctypes.data, 0, p.n, p.k, p.level,
                                                          p.N), "convert_bsk_generic")
        r = torch.zeros(1, dtype=torch.int64, device=DEV)
        out = filled(env, (batch + 1, p.lwe_out_size))
        d_in, d_acc = B.to_device(c["cts"], DEV), B.to_device(c["acc"][None, :], DEV)
        env["N"].check(L.concrete_hip_pbs_generic(st, 0, out.data_ptr(), None, d_acc.data_ptr(), None, d_in.data_ptr(),
                                                  None, g.data_ptr(), p.n, p.k, p.N, p.base_log, p.level, batch,
                                                  r.data_ptr()), "pbs_generic")
        torch.cuda.synchronize()
        assert B.stream_status(DEV) == 0
        return dict(via_keyset=via_keyset, out=B.to_host(out), resid=resid_bits(r), key=B.to_host(g),
                    max_g=L.concrete_hip_key_spectrum_max(g.data_ptr()))

    clean, got = both(monkeypatch, fill, "companion", run)
    for res in (clean, got):
        assert np.array_equal(res["via_keyset"], c["ref"]), "the companion key's run differs from the oracle"
        assert np.array_equal(res["out"][:batch], c["ref"]), "the caller-converted key's run differs from the oracle"
        assert (res["out"][batch] == np.uint64(SENTINEL)).all()
    assert np.array_equal(got["key"], clean["key"]) and got["max_g"] == clean["max_g"] > 0
    assert got["resid"] == clean["resid"]
    # (concrete_hip_generic_error_bound answers only where the primary key format is the general one)
    bound = V.error_bound(p.k, p.N, p.level, p.base_log, clean["max_g"])
    assert 0.0 <= as_f64(got["resid"]) < bound < 0.5, (as_f64(got["resid"]), bound)


# ---------------------------------------------------------------------------------------------------------
# 2.2 the keyswitch's matrix-core path
# ---------------------------------------------------------------------------------------------------------
# n_in = 40, (l, logB) = (4, 3), n_out = 630, batch 129: W = 631 of NP = 640 columns, rows 129 .. 255 of the row
# tile past the batch; (7, 3) at n_in = 1024: K split over workgroups, outputs zeroed first and added atomically.
# (id, n_in, l, logB, batch, CONCRETE_HIP_KS_CHUNK, key in a cuda_malloc_async buffer)
KS_ROWS = [
    ("ragged_tiles", 40, 4, 3, 129, None, False),
    ("two_passes", 40, 4, 3, 129, "128", False),
    ("cached_key_bytes", 40, 4, 3, 129, None, True),
    ("split_k", 1024, 7, 3, 129, None, False),
]


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("row", KS_ROWS, ids=[r[0] for r in KS_ROWS])
def test_keyswitch_matrix_core_path(env, monkeypatch, row, fill):
    """A key in a torch tensor: the key bytes come from the pool with every call; in a cuda_malloc_async buffer:
    from the cached branch, built under the fill by the first call (the buffer is new per run)."""
    B, O, torch = env["B"], env["O"], env["torch"]
    name, n_in, ks_l, ks_logB, nb, chunk, runtime_key = row
    p = B.PbsParams(n=630, k=1, N=n_in, level=1, base_log=1, ks_level=ks_l, ks_base_log=ks_logB)

    def make():
        ksk = B.ksk_generate(p, B.binary_key(p.big_n, 8800 + n_in), B.binary_key(p.n, 8801 + n_in), 8802 + n_in)
        rng = np.random.RandomState(nb + n_in)
        cts = rng.randint(0, 2 ** 63, size=(nb, p.big_n + 1), dtype=np.int64).astype(np.uint64) * np.uint64(2) + \
            np.uint64(1)
        cts[0] = 0
        cts[1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        op = O.Params(n=p.n, k=p.k, N=p.N, l=p.level, logB=p.base_log, ks_l=ks_l, ks_logB=ks_logB)
        return dict(ksk=ksk, cts=cts, ref=O.keyswitch_batch(op, cts, ksk))

    c = once(("ks", n_in), make)
    if chunk:
        monkeypatch.setenv("CONCRETE_HIP_KS_CHUNK", chunk)

    def run(_):
        key = B.RuntimeBuffer(c["ksk"]) if runtime_key else B.to_device(c["ksk"], DEV)
        try:
            out = filled(env, (nb + 1, p.n + 1))
            B.keyswitch(p, key, B.to_device(c["cts"], DEV), out=out, num_samples=nb)
            again = B.keyswitch(p, key, B.to_device(c["cts"], DEV))  # the cached key bytes, where there are any
            torch.cuda.synchronize()
            return B.to_host(out), B.to_host(again)
        finally:
            if runtime_key:
                key.free()

    clean, got = both(monkeypatch, fill, ("ks", name), run)
    for out, again in (clean, got):
        assert np.array_equal(out[:nb], c["ref"]), f"{int((out[:nb] != c['ref']).sum())} words differ from the oracle"
        assert (out[nb] == np.uint64(SENTINEL)).all(), "wrote past the output"
        assert np.array_equal(again, c["ref"])
    assert np.array_equal(got[0], clean[0])


# ---------------------------------------------------------------------------------------------------------
# 2.3 key conversion
# ---------------------------------------------------------------------------------------------------------
# (id, k, N, l, logB, n, general format): every hand-tuned key kind, the general format (of a general-path shape
# and of a hand-tuned ring: the companion's), the split format
KEY_ROWS = [
    ("n1024", 1, 1024, 3, 7, 4, False),
    ("n2048", 1, 2048, 1, 23, 4, False),
    ("k2n1024", 2, 1024, 1, 23, 3, False),
    ("small_k3n512", 3, 512, 1, 18, 4, False),
    ("small_k4n512_l2", 4, 512, 2, 16, 3, False),
    ("small_k6n256", 6, 256, 1, 18, 3, False),
    ("general_k3n512_l4", 3, 512, 4, 9, 3, False),
    ("general_n8192", 1, 8192, 1, 22, 3, False),
    ("general_of_n1024", 1, 1024, 1, 23, 4, True),
    ("split_n32768", 1, 32768, 2, 15, 2, False),
]
KEY_KINDS = {"n1024": 1, "n2048": 2, "k2n1024": 4, "small_k3n512": 5, "small_k4n512_l2": 5, "small_k6n256": 5,
             "general_k3n512_l4": 3, "general_n8192": 3, "general_of_n1024": 1, "split_n32768": 3}


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("row", KEY_ROWS, ids=[r[0] for r in KEY_ROWS])
def test_key_conversion(env, monkeypatch, row, fill):
    """The Fourier key converted from a host key under the fill equals the clean conversion byte for byte, and so
    does the recorded spectrum maximum.  (That the clean key is the right one: tests/test_gpu_key_accuracy.py.)"""
    B, L, torch = env["B"], env["L"], env["torch"]
    name, k, N, l, logB, n, general = row
    p = B.PbsParams(n=n, k=k, N=N, level=l, base_log=logB)
    assert B.bsk_format(p)[0] == KEY_KINDS[name]
    bsk = once(("key", name), lambda: B.bsk_generate(p, B.binary_key(p.n, 8900), B.binary_key(p.big_n, 8901), 8902))

    def run(_):
        st = B._stream(DEV)
        if general:
            dest = torch.zeros(L.concrete_hip_generic_bsk_size_bytes(n, k, l, N) // 8, dtype=torch.int64, device=DEV)
            env["N"].check(L.concrete_hip_convert_bsk_generic(st, 0, dest.data_ptr(), bsk.ctypes.data, 0, n, k, l, N),
                           "convert_bsk_generic")
        else:
            dest = torch.zeros(B.fourier_bsk_bytes(p) // 8, dtype=torch.int64, device=DEV)
            B.convert_bsk(p, bsk, DEV, out=dest)
        torch.cuda.synchronize()
        return B.to_host(dest), L.concrete_hip_key_spectrum_max(dest.data_ptr())

    (clean_key, clean_max), (key, max_g) = both(monkeypatch, fill, ("key", name), run)
    assert clean_key.size > 0 and clean_key.any() and clean_max > 0.0
    assert np.array_equal(key, clean_key), f"{int((key != clean_key).sum())} of {key.size} key words differ"
    assert max_g == clean_max


# ---------------------------------------------------------------------------------------------------------
# 2.4 caller-provided scratch: exactly the queried size, every byte the fill, a guard behind it
# ---------------------------------------------------------------------------------------------------------
EB_ROWS, EB_NB, EB_DL = 5, 4, 60  # test_gpu_extract_bits.test_bit_exact_against_oracle's, at cfg2's ring and n = 8


def _eb_case(env):
    def make():
        te = env["te"]
        S = TE._setup(te, "cfg2")
        pts = TE._plaintexts(np.random.RandomState(11), [EB_NB] * EB_ROWS, [EB_DL] * EB_ROWS)
        cts = TE._encrypt_big(te, S, pts, 7201)
        return dict(S=S, cts=cts, ref=TE._oracle_extract(te, S, cts, [EB_NB] * EB_ROWS, [EB_DL] * EB_ROWS))
    return once("extract_bits", make)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_extract_bits_on_callers_scratch(env, monkeypatch, fill):
    B, torch = env["B"], env["torch"]
    c = _eb_case(env)
    S = c["S"]
    p, total = S["p"], EB_ROWS * EB_NB

    def run(f):
        scratch, guard = callers_scratch(env, B.extract_bits_scratch_bytes(p, EB_ROWS, EB_NB), f)
        out = filled(env, (total + 1, p.n + 1))
        B.extract_bits(p, S["fbsk"], S["ksk_dev"], B.to_device(c["cts"], DEV), EB_NB, EB_DL, out=out, scratch=scratch)
        torch.cuda.synchronize()
        assert B.stream_status(DEV) == 0 and guard_intact(guard), "wrote past the scratch buffer"
        return B.to_host(out)

    clean, got = both(monkeypatch, fill, "extract_bits", run)
    for out in (clean, got):
        assert np.array_equal(out[:total], c["ref"]), f"{int((out[:total] != c['ref']).sum())} words differ"
        assert (out[total] == np.uint64(SENTINEL)).all()


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_extract_bits_reference_names(env, monkeypatch, fill):
    """scratch_cuda_extract_bits_64's buffer (filled by the hook) into cuda_extract_bits_64."""
    L, B, torch = env["L"], env["B"], env["torch"]
    c = _eb_case(env)
    S = c["S"]
    p, total = S["p"], EB_ROWS * EB_NB
    monkeypatch.setenv(KNOB, hex(fill))
    s = B._stream(DEV)
    out = filled(env, (total + 1, p.n + 1))
    d_in = B.to_device(c["cts"], DEV)
    buf = C.c_void_p(None)
    L.scratch_cuda_extract_bits_64(s, 0, C.byref(buf), p.k, p.n, p.N, p.level, EB_ROWS, 0, True)
    assert buf.value
    L.cuda_extract_bits_64(s, 0, out.data_ptr(), d_in.data_ptr(), buf, S["ksk_dev"].data_ptr(), S["fbsk"].data_ptr(),
                           EB_NB, EB_DL, p.big_n, p.n, p.k, p.N, p.base_log, p.level, p.ks_base_log, p.ks_level, EB_ROWS,
                           0)
    L.cleanup_cuda_extract_bits(s, 0, C.byref(buf))
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got = B.to_host(out)
    assert np.array_equal(got[:total], c["ref"]) and (got[total] == np.uint64(SENTINEL)).all()


CBS_SHAPE, CBS_LEVEL, CBS_SAMPLES, CBS_DL = "n512", 2, 3, 59  # the run of CBS_RUNS that takes the caller's scratch


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_circuit_bootstrap_on_callers_scratch(env, monkeypatch, fill):
    B, torch = env["B"], env["torch"]
    _, _, (pl, pb), cb, _ = TC.CBS_SHAPES[CBS_SHAPE]
    e = TC._cbs_keys(env["tc"], CBS_SHAPE)
    c = TC._cbs_case(env["tc"], CBS_SHAPE, CBS_DL)
    p, samples, lv = e["p"], CBS_SAMPLES, CBS_LEVEL
    want_ggsw, want_w = c["ggsw"][:samples, :lv], c["w"][:samples, :lv]

    def run(f):
        scratch, guard = callers_scratch(env, B.circuit_bootstrap_scratch_bytes(p, lv, samples), f)
        out = filled(env, (samples + 1, lv, p.k + 1, p.glwe_size))
        w = filled(env, (samples + 1, lv, p.big_n + 1))
        B.circuit_bootstrap(p, e["fbsk"], e["d_fpksk"], B.to_device(c["cts"][:samples].copy(), DEV), CBS_DL, pl, pb, lv,
                            cb, out=out, scratch=scratch, pbs_out=w)
        torch.cuda.synchronize()
        assert B.stream_status(DEV) == 0 and guard_intact(guard), "wrote past the scratch buffer"
        return B.to_host(out), B.to_host(w)

    clean, got = both(monkeypatch, fill, "cbs", run)
    for out, w in (clean, got):
        assert np.array_equal(w[:samples], want_w), "the rows after the PBS differ (before the fp-ks)"
        assert np.array_equal(out[:samples], want_ggsw), "the GGSWs differ (in the fp-ks)"
        assert (w[samples] == np.uint64(SENTINEL)).all() and (out[samples] == np.uint64(SENTINEL)).all()


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_circuit_bootstrap_reference_names(env, monkeypatch, fill):
    L, B, torch = env["L"], env["B"], env["torch"]
    (k, N, n), (bl, bb), (pl, pb), cb, _ = TC.CBS_SHAPES[CBS_SHAPE]
    e = TC._cbs_keys(env["tc"], CBS_SHAPE)
    c = TC._cbs_case(env["tc"], CBS_SHAPE, CBS_DL)
    samples, lv = CBS_SAMPLES, CBS_LEVEL
    monkeypatch.setenv(KNOB, hex(fill))
    s = B._stream(DEV)
    d_in = B.to_device(c["cts"][:samples].copy(), DEV)
    out = filled(env, (samples + 1, lv, k + 1, (k + 1) * N))
    buf = C.c_void_p(None)
    L.scratch_cuda_circuit_bootstrap_64(s, 0, C.byref(buf), k, n, N, lv, samples, 0, True)
    assert buf.value
    L.cuda_circuit_bootstrap_64(s, 0, out.data_ptr(), d_in.data_ptr(), e["fbsk"].data_ptr(), e["d_fpksk"].data_ptr(), None,
                                buf, CBS_DL, N, k, n, bl, bb, pl, pb, lv, cb, samples, 0)
    L.cleanup_cuda_circuit_bootstrap(s, 0, C.byref(buf))
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got = B.to_host(out)
    assert np.array_equal(got[:samples], c["ggsw"][:samples, :lv]) and (got[samples] == np.uint64(SENTINEL)).all()


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_fp_keyswitch(env, monkeypatch, fill):
    """The call takes no scratch argument: its split sums and the packing's staging are the pool's."""
    B, torch = env["B"], env["torch"]
    (k, N), (level, base_log) = TC.FPKS_SHAPES[0], TC.FPKS_DECOMP[1]
    c = TC._fpks_case(env["tc"], k, N, level, base_log)
    rows, G = TC.T + 1, (k + 1) * N

    def run(_):
        out = filled(env, (rows + 1, k + 1, G))
        B.fp_keyswitch(k, N, level, base_log, c["d_key"], B.to_device(c["rows"][:rows].copy(), DEV), out=out)
        torch.cuda.synchronize()
        return B.to_host(out)

    clean, got = both(monkeypatch, fill, "fpks", run)
    for out in (clean, got):
        assert np.array_equal(out[:rows], c["want"][:rows]) and (out[rows] == np.uint64(SENTINEL)).all()


VP_SHAPE, VP_GEOM = "n512", (3, 4, 3, 3)  # the geometry of test_gpu_vertical_packing that takes the caller's scratch


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_vertical_packing_on_callers_scratch(env, monkeypatch, fill):
    B, torch = env["B"], env["torch"]
    c = TV._case(env["tv"], VP_SHAPE, VP_GEOM)
    p = c["p"]

    def run(f):
        scratch, guard = callers_scratch(env, B.vertical_packing_scratch_bytes(p, *VP_GEOM), f)
        resid = torch.zeros(1, dtype=torch.int64, device=DEV)
        lwe, tree, max_g = TV._run(env["tv"], c, VP_GEOM, scratch=scratch, resid=resid)
        assert B.stream_status(DEV) == 0 and guard_intact(guard), "wrote past the scratch buffer"
        return lwe, tree, max_g, resid_bits(resid)

    clean, got = both(monkeypatch, fill, "vp", run)
    for lwe, tree, _, _ in (clean, got):
        assert np.array_equal(tree, c["tree"]), "the CMUX tree's result differs from the reference"
        assert np.array_equal(lwe, c["lwe"]), "the extracted LWEs differ from the reference"
    assert got[2] == clean[2] > 0.0 and got[3] == clean[3]
    bound = V.error_bound(p.k, p.N, p.level, p.base_log, clean[2])
    assert 0.0 < as_f64(got[3]) <= bound < 0.5


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_vertical_packing_reference_names(env, monkeypatch, fill):
    """cuda_cmux_tree_64 into cuda_blind_rotate_and_sample_extraction_64, each on its scratch call's buffer."""
    L, B, torch = env["L"], env["B"], env["torch"]
    c = TV._case(env["tv"], VP_SHAPE, VP_GEOM)
    p = c["p"]
    r, m, tau, _ = VP_GEOM
    words = V.ggsw_words(p.k, p.N, p.level)
    monkeypatch.setenv(KNOB, hex(fill))
    d_ggsw = B.to_device(c["ggsws"][0].reshape(-1).copy(), DEV)  # lookup 0
    d_luts = B.to_device(c["luts"].copy(), DEV)
    glwe, lwe = filled(env, (tau + 1, p.glwe_size)), filled(env, (tau + 1, p.lwe_out_size))
    s = B._stream(DEV)
    buf = C.c_void_p(None)
    L.scratch_cuda_cmux_tree_64(s, 0, C.byref(buf), p.k, p.N, p.level, r, tau, 0, True)
    assert buf.value
    L.cuda_cmux_tree_64(s, 0, glwe.data_ptr(), d_ggsw.data_ptr(), d_luts.data_ptr(), buf, p.k, p.N, p.base_log, p.level, r,
                        tau, 0)
    L.cleanup_cuda_cmux_tree(s, 0, C.byref(buf))
    L.scratch_cuda_blind_rotation_sample_extraction_64(s, 0, C.byref(buf), p.k, p.N, p.level, m, tau, 0, True)
    L.cuda_blind_rotate_and_sample_extraction_64(s, 0, lwe.data_ptr(), d_ggsw.data_ptr() + 8 * r * words, glwe.data_ptr(),
                                                 buf, m, tau, p.k, p.N, p.base_log, p.level, 0)
    L.cleanup_cuda_blind_rotation_sample_extraction(s, 0, C.byref(buf))
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    g, w = B.to_host(glwe), B.to_host(lwe)
    assert np.array_equal(g[:tau], c["tree"][0]) and (g[tau] == np.uint64(SENTINEL)).all()
    assert np.array_equal(w[:tau], c["lwe"][0]) and (w[tau] == np.uint64(SENTINEL)).all()


WOP_MODULI, WOP_BATCH = Cs.MODULI_SETS[0], 2


def _wop_keys(env):
    def make():
        B, k = env["B"], Cs.keys()
        d = dict(keys=k, fbsk=B.convert_bsk(Cs.P, k["bsk"], DEV), d_ksk=B.to_device(k["ksk"].copy(), DEV),
                 d_fpksk=B.to_device(k["fpksk"].reshape(-1).copy(), DEV))
        env["torch"].cuda.synchronize()
        return d
    return once("wop_keys", make)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_wop_pbs_crt_on_callers_scratch(env, monkeypatch, fill):
    B, torch = env["B"], env["torch"]
    K, c = _wop_keys(env), Cs.case(WOP_MODULI)
    nblk, batch, width = len(WOP_MODULI), WOP_BATCH, Cs.K * Cs.N + 1
    assert B.wop_pbs_supported(Cs.P, *Cs.PKSK, *Cs.CBS)

    def run(f):
        scratch, guard = callers_scratch(env, B.wop_pbs_scratch_bytes(Cs.P, Cs.CBS[0], nblk, c["t"], nblk, batch), f)
        out = filled(env, (batch + 1, nblk, width))
        _, max_g = B.wop_pbs_crt(Cs.P, K["fbsk"], K["d_ksk"], K["d_fpksk"], B.to_device(c["blocks"][:batch].copy(), DEV),
                                 B.to_device(c["luts"].copy(), DEV), WOP_MODULI, *Cs.PKSK, *Cs.CBS, out=out,
                                 scratch=scratch)
        torch.cuda.synchronize()
        assert B.stream_status(DEV) == 0 and guard_intact(guard), "wrote past the scratch buffer"
        return B.to_host(out), max_g

    clean, got = both(monkeypatch, fill, "wop_crt", run)
    for out, _ in (clean, got):
        assert np.array_equal(out[:batch], c["want"][:batch]) and (out[batch] == np.uint64(SENTINEL)).all()
    assert got[1] == clean[1] > 0.0


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_circuit_bootstrap_vertical_packing_on_callers_scratch(env, monkeypatch, fill):
    """Stages 2 and 3 in one call on the reference's extracted bits of the same values."""
    B, torch = env["B"], env["torch"]
    K, c = _wop_keys(env), Cs.case(WOP_MODULI)
    nblk, batch, width = len(WOP_MODULI), WOP_BATCH, Cs.K * Cs.N + 1
    k = K["keys"]
    bits = once("wop_bits", lambda: W.crt_extract(c["blocks"][:batch], WOP_MODULI, k["bsk"], k["ksk"], Cs.OP))

    def run(f):
        scratch, guard = callers_scratch(env, B.wop_pbs_scratch_bytes(Cs.P, Cs.CBS[0], 0, c["t"], nblk, batch), f)
        out = filled(env, (batch + 1, nblk, width))
        _, max_g = B.circuit_bootstrap_vertical_packing(Cs.P, K["fbsk"], K["d_fpksk"], B.to_device(bits, DEV),
                                                        B.to_device(c["luts"].copy(), DEV), *Cs.PKSK, *Cs.CBS, out=out,
                                                        scratch=scratch)
        torch.cuda.synchronize()
        assert B.stream_status(DEV) == 0 and guard_intact(guard), "wrote past the scratch buffer"
        return B.to_host(out), max_g

    clean, got = both(monkeypatch, fill, "cbs_vp", run)
    for out, _ in (clean, got):
        assert np.array_equal(out[:batch], c["want"][:batch]) and (out[batch] == np.uint64(SENTINEL)).all()
    assert got[1] == clean[1] > 0.0


NAMED_INPUTS, NAMED_BITS, NAMED_WITH_PADDING = 2, 3, 4  # test_gpu_wop_pbs.py's reference-named lookup


def _named(env):
    """Two inputs of 3 message bits under a padding bit, the LUTs in the reference-named layout, the CPU reference's
    bits and outputs of the one lookup."""
    def make():
        B, k = env["B"], Cs.keys()
        delta_log, t = 64 - NAMED_WITH_PADDING, NAMED_INPUTS * NAMED_BITS
        cts = B.lwe_encrypt(k["glwe_sk"], np.array([v << delta_log for v in (5, 3)], dtype=np.uint64), Cs.K * Cs.N,
                            Cs.INPUT_STD, 9971)
        table = np.random.RandomState(9972).randint(0, 1 << Cs.WIDTH, size=(NAMED_INPUTS, 1 << t)).astype(np.uint64)
        luts = table << np.uint64(64 - Cs.WIDTH)
        padded = W.lut_layout(luts, t, Cs.N).reshape(NAMED_INPUTS, Cs.N)
        bits = W.extract_bits(cts, k["bsk"], k["ksk"], [NAMED_BITS] * NAMED_INPUTS, [delta_log] * NAMED_INPUTS,
                              [0, NAMED_BITS], Cs.OP)
        want = W.cbs_vp(bits[None], luts, k["bsk"], k["fpksk"], Cs.OP, Cs.PKSK, Cs.CBS)[0]
        return dict(cts=cts, padded=padded, bits=bits, want=want, delta_log=delta_log, t=t)
    return once("named", make)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_wop_pbs_reference_names(env, monkeypatch, fill):
    """cuda_wop_pbs_64 and cuda_circuit_bootstrap_vertical_packing_64, each on its scratch call's buffer."""
    L, B, torch = env["L"], env["B"], env["torch"]
    K, nm = _wop_keys(env), _named(env)
    n_in, width = NAMED_INPUTS, Cs.K * Cs.N + 1
    (bl, bb), (kl, kb), (pl, pb), (cl, cb) = Cs.BSK, Cs.KS, Cs.PKSK, Cs.CBS
    monkeypatch.setenv(KNOB, hex(fill))
    s = B._stream(DEV)
    d_cts, d_bits, d_padded = (B.to_device(nm[x], DEV) for x in ("cts", "bits", "padded"))
    buf, dl, cdl = C.c_void_p(None), C.c_uint32(0), C.c_uint32(0)
    L.scratch_cuda_wop_pbs_64(s, 0, C.byref(buf), C.byref(dl), C.byref(cdl), Cs.K, Cs.LWE_N, Cs.N, cl, bl,
                              NAMED_WITH_PADDING, NAMED_BITS, n_in, 0, True)
    assert buf.value and (dl.value, cdl.value) == (nm["delta_log"], 63)
    out = filled(env, (n_in + 1, width))
    L.cuda_wop_pbs_64(s, 0, out.data_ptr(), d_cts.data_ptr(), d_padded.data_ptr(), K["fbsk"].data_ptr(),
                      K["d_ksk"].data_ptr(), K["d_fpksk"].data_ptr(), buf, cdl.value, Cs.K, Cs.LWE_N, Cs.N, bb, bl, kb, kl,
                      pb, pl, cb, cl, NAMED_WITH_PADDING, NAMED_BITS, dl.value, n_in, 0)
    L.cleanup_cuda_wop_pbs(s, 0, C.byref(buf))
    out2 = filled(env, (n_in + 1, width))
    L.scratch_cuda_circuit_bootstrap_vertical_packing_64(s, 0, C.byref(buf), C.byref(cdl), Cs.K, Cs.LWE_N, Cs.N, cl,
                                                         nm["t"], n_in, 0, True)
    assert buf.value and cdl.value == 63
    L.cuda_circuit_bootstrap_vertical_packing_64(s, 0, out2.data_ptr(), d_bits.data_ptr(), K["fbsk"].data_ptr(),
                                                 K["d_fpksk"].data_ptr(), d_padded.data_ptr(), buf, cdl.value, Cs.N, Cs.K,
                                                 Cs.LWE_N, bl, bb, pl, pb, cl, cb, nm["t"], n_in, 0)
    L.cleanup_cuda_circuit_bootstrap_vertical_packing(s, 0, C.byref(buf))
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    for o in (B.to_host(out), B.to_host(out2)):
        assert np.array_equal(o[:n_in], nm["want"]) and (o[n_in] == np.uint64(SENTINEL)).all()


# ---------------------------------------------------------------------------------------------------------
# 2.5 the runtime glue: slice staging buffers
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_batched_bootstrap_on_three_slices(env, monkeypatch, fill):
    """tests/test_gpu_runtime.py test_batched_bootstrap: batch 7 on three slices of device 0, twice per keyset (new
    staging buffers, then reused ones: the hook fills both)."""
    B, O, RT = env["B"], env["O"], env["RT"]
    p = replace(B.CFG2, n=24)
    width, nb = 3, 7

    def make():
        op = O.Params(n=p.n, k=p.k, N=p.N, l=p.level, logB=p.base_log, ks_l=p.ks_level, ks_logB=p.ks_base_log)
        lwe_sk, glwe_sk = B.binary_key(p.n, 71), B.binary_key(p.big_n, 72)
        bsk = B.bsk_generate(p, lwe_sk, glwe_sk, 73)
        tlu = B.expand_lut(np.array([2, 7, 1, 0, 5, 5, 3, 6], dtype=np.uint64), p.N, width)
        msgs = np.random.RandomState(107).randint(0, 1 << width, size=nb)
        cts = B.lwe_encrypt(lwe_sk, [B.encode(m, width) for m in msgs], p.n, 2.0 ** -25, 107)
        ref, _ = O.pbs_batch(op, cts, B.trivial_glwe(p, tlu)[None, :], fbsk=O.bsk_to_fourier(op, bsk))
        return dict(bsk=bsk, tlu=tlu, cts=cts, ref=ref)

    c = once("runtime", make)

    def run(_):
        ks = RT.Keyset([0, 0, 0])
        ks.add_bsk(0, c["bsk"], p)
        try:
            return RT.batched_bootstrap(ks, p, c["cts"], c["tlu"]), RT.batched_bootstrap(ks, p, c["cts"], c["tlu"])
        finally:
            ks.close()

    clean, got = both(monkeypatch, fill, "runtime", run)
    for res in clean + got:
        assert np.array_equal(res, c["ref"])


SDFG_CTX = 0x5DF7  # the runtime-context pointer this file's keyset is bound to


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_sdfg_keyswitch_bootstrap_add(env, monkeypatch, fill):
    """A stream-emulator graph x -> KS -> s, s -> PBS(lut) -> b, add(b, y) -> o at batch 7 (the graph builder and
    the host model of tests/test_gpu_sdfg_graph.py); o is read twice (new staging buffers, then reused ones)."""
    RT = env["RT"]
    batch = 7
    TS.set_devices(monkeypatch, None)

    def make():
        K = TS.keys0(SDFG_CTX)
        rng = np.random.RandomState(4300)
        msgs = rng.randint(0, 1 << TS.WIDTH, size=batch)
        x = TS.encrypt(K, K.glwe_sk, msgs, 4301)
        y = TS.words(rng, batch, K.p.big_n + 1)
        lut = K.lut(rng.randint(0, 1 << TS.WIDTH, size=1 << TS.WIDTH))
        return dict(K=K, x=x, y=y, lut=lut, want=TS.op_add(K.bootstrap(K.keyswitch(x), lut), y))

    c = once("sdfg", make)
    K = c["K"]

    def run(_):
        kset = RT.Keyset([0])
        kset.add_bsk(0, K.bsk, K.p)
        kset.add_ksk(0, K.ksk, K.pks)
        kset.bind(SDFG_CTX)
        G = TS.Graph(RT)
        try:
            G.inputs("x", "y")
            G.inputs("lut", kind="memref")
            G.stream("s")
            G.stream("b")
            G.stream("o", stype=TS.TS_TOPO_TO_X86)
            G.keyswitch("x", "s", K)
            G.bootstrap("s", "lut", "b", K)
            G.linear("add", "b", "y", "o")
            outs = []
            for _ in range(2):
                for name in ("x", "y", "lut"):
                    G.put(name, c[name])
                outs.append(G.g.get_batch(G.h["o"], *c["want"].shape))
            return outs
        finally:
            G.close()
            kset.close()

    clean, got = both(monkeypatch, fill, "sdfg", run)
    for o in clean + got:
        assert np.array_equal(o, c["want"]), f"{int((o != c['want']).sum())} of {o.size} words differ"
