"""GPU tests of the chained WoP-PBS (concrete_amd/csrc/wop_pbs.hip): the CRT batch call, stages 2
and 3 in one call, the reference-named triples and the memref routes.

The definition is tests/wop_reference.py (the CRT front, the extraction loop on the oracle's integer keyswitch and
PBS, cbs_reference, the LUT layout, vp_reference).  The device computes the same integers, so every comparison is
word for word; there is no tolerance anywhere.  Outputs are sentinel-filled before each call and carry one row
more than the call writes, which must keep the sentinel.  The small cases (shape A) and their reference live in
tests/wop_cases.py, made once; tests/test_wop_pbs_abi.py settles their decryption margin on the CPU.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_shapes as S  # noqa: E402
import wop_cases as Cs  # noqa: E402
import wop_reference as W  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
IDS = lambda m: "x".join(map(str, m))  # noqa: E731


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from concrete_amd import _native
    from concrete_amd import backend as B
    from concrete_amd import runtime as RT
    k = Cs.keys()
    e = dict(torch=torch, L=_native.lib(), B=B, RT=RT, keys=k, fbsk=B.convert_bsk(Cs.P, k["bsk"], DEV),
             d_ksk=B.to_device(k["ksk"].copy(), DEV), d_fpksk=B.to_device(k["fpksk"].reshape(-1).copy(), DEV))
    torch.cuda.synchronize()
    return e


def _rand_u64(rng, shape):
    return rng.randint(0, 1 << 32, size=shape).astype(np.uint64) << np.uint64(32) | \
        rng.randint(0, 1 << 32, size=shape).astype(np.uint64)


def _filled(env, shape):
    t = env["torch"].empty(shape, dtype=env["torch"].int64, device=DEV)
    t.fill_(SENTINEL)  # below 2^63: the same bits as int64
    return t


def _crt_a(env, moduli, batch, own_scratch=False):
    """concrete_hip_wop_pbs_crt at shape A on the first `batch` values of the case: (output words, max|G|)."""
    B, torch = env["B"], env["torch"]
    c = Cs.case(moduli)
    nblk, width = len(moduli), Cs.K * Cs.N + 1
    assert B.wop_pbs_supported(Cs.P, *Cs.PKSK, *Cs.CBS)
    d_in = B.to_device(c["blocks"][:batch].copy(), DEV)
    d_luts = B.to_device(c["luts"].copy(), DEV)
    out = _filled(env, (batch + 1, nblk, width))  # one value's rows more than the call writes
    scratch = guard = None
    if own_scratch:  # the caller's scratch, exactly the size the query names, and a guard right behind it
        need = B.wop_pbs_scratch_bytes(Cs.P, Cs.CBS[0], nblk, c["t"], nblk, batch)
        assert need > 0 and need % 16 == 0
        buf = _filled(env, (need // 8 + 4096,))
        scratch, guard = buf[:need // 8], buf[need // 8:]
        assert scratch.data_ptr() % 16 == 0 and scratch.numel() * 8 == need
    _, max_g = B.wop_pbs_crt(Cs.P, env["fbsk"], env["d_ksk"], env["d_fpksk"], d_in, d_luts, moduli, *Cs.PKSK, *Cs.CBS,
                             out=out, scratch=scratch)
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got = B.to_host(out)
    assert (got[batch] == np.uint64(SENTINEL)).all(), "wrote past the output"
    assert np.array_equal(B.to_host(d_in), c["blocks"][:batch]), "the input was modified"
    if guard is not None:
        assert (B.to_host(guard) == np.uint64(SENTINEL)).all(), "wrote past the scratch buffer"
    assert max_g > 0.0
    return got[:batch]


# ---------------------------------------------------------------------------------------------------------
# shape A: the CRT batch call against the CPU reference
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (1, Cs.BATCH))
@pytest.mark.parametrize("moduli", Cs.MODULI_SETS, ids=IDS)
def test_wop_pbs_crt_equals_the_reference_and_decrypts(env, moduli, batch):
    c = Cs.case(moduli)
    nblk = len(moduli)
    got = _crt_a(env, moduli, batch)
    assert np.array_equal(got, c["want"][:batch])
    # the outputs decrypt to the random table's entries (2-bit messages at the top of the word)
    want = [int(c["table"][o, c["index"][b]]) for b in range(batch) for o in range(nblk)]
    assert Cs.messages(Cs.decrypt(got.reshape(-1, Cs.K * Cs.N + 1))) == want


@pytest.mark.parametrize("moduli", Cs.MODULI_SETS, ids=IDS)
def test_callers_scratch_of_exactly_the_queried_size(env, moduli):
    got = _crt_a(env, moduli, 2, own_scratch=True)
    assert np.array_equal(got, Cs.case(moduli)["want"][:2])


def test_stages_2_and_3_in_one_call_equal_the_reference(env):
    """concrete_hip_circuit_bootstrap_vertical_packing on the reference's extracted bits of [5, 7, 8, 9]."""
    B, torch = env["B"], env["torch"]
    moduli, k = Cs.MODULI_SETS[2], env["keys"]
    c = Cs.case(moduli)
    bits = W.crt_extract(c["blocks"][:2], moduli, k["bsk"], k["ksk"], Cs.OP)
    out = _filled(env, (3, len(moduli), Cs.K * Cs.N + 1))
    B.circuit_bootstrap_vertical_packing(Cs.P, env["fbsk"], env["d_fpksk"], B.to_device(bits, DEV),
                                         B.to_device(c["luts"].copy(), DEV), *Cs.PKSK, *Cs.CBS, out=out)
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got = B.to_host(out)
    assert np.array_equal(got[:2], c["want"][:2])
    assert (got[2] == np.uint64(SENTINEL)).all()


# ---------------------------------------------------------------------------------------------------------
# shape B: the WoP table's ring, against the composition of the backend's own three public stage calls
# ---------------------------------------------------------------------------------------------------------
RING_K, RING_N = S.WOP_RING
COMBOS = S.distinct(S.WOP_ROWS, "br_l", "br_b", "ks_l", "ks_b", "pp_l", "pp_b", "cb_l", "cb_b")
BR_L, BR_B, KS_L, KS_B, PP_L, PP_B, CB_L, CB_B = min(COMBOS, key=lambda q: (q[4], q))  # the fewest fp-ks levels


@pytest.fixture(scope="module")
def ring(env):
    B, torch = env["B"], env["torch"]
    p = B.PbsParams(n=8, k=RING_K, N=RING_N, level=BR_L, base_log=BR_B, ks_level=KS_L, ks_base_log=KS_B)
    lwe_sk, glwe_sk = B.binary_key(p.n, 9951), B.binary_key(p.big_n, 9952)
    bsk = B.bsk_generate(p, lwe_sk, glwe_sk, 9953, std=Cs.KEY_STD)
    ksk = B.ksk_generate(p, glwe_sk, lwe_sk, 9954, std=Cs.KEY_STD)
    fpksk = _rand_u64(np.random.RandomState(9955), (p.k + 1) * (p.big_n + 1) * PP_L * p.glwe_size)
    r = dict(p=p, glwe_sk=glwe_sk, fbsk=B.convert_bsk(p, bsk, DEV), d_ksk=B.to_device(ksk, DEV),
             d_fpksk=B.to_device(fpksk, DEV))
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("moduli", ((4, 4), (8, 16, 16)), ids=IDS)  # t = 4: padding; t = 11: r = 1, m = 10
def test_table_ring_equals_the_three_stage_calls(env, ring, moduli):
    B, torch = env["B"], env["torch"]
    p, batch, nblk = ring["p"], 2, len(moduli)
    assert B.wop_pbs_supported(p, PP_L, PP_B, CB_L, CB_B)
    t = sum(W.crt_bits(m) for m in moduli)
    r, m = W.rm(t, p.N)
    assert (t, r, m) in ((4, 0, 4), (11, 1, 10))
    rng = np.random.RandomState(9960 + t)
    values = [0] + [int(v) for v in rng.randint(1, int(np.prod(moduli)), size=batch - 1)]
    pts = np.array([W.crt_encode(v, q) for v in values for q in moduli], dtype=np.uint64)
    blocks = B.lwe_encrypt(ring["glwe_sk"], pts, p.big_n, Cs.INPUT_STD, 9961 + t).reshape(batch, nblk, p.big_n + 1)
    luts = _rand_u64(rng, (nblk, 1 << t))
    d_in = B.to_device(blocks, DEV)
    # the composition: the three public stage calls, the LUT laid out on the host
    bits = B.crt_extract_bits(p, ring["fbsk"], ring["d_ksk"], d_in, moduli)
    ggsw = B.circuit_bootstrap(p, ring["fbsk"], ring["d_fpksk"], bits.reshape(batch * t, p.n + 1).contiguous(), 63,
                               PP_L, PP_B, CB_L, CB_B)
    vp = B.PbsParams(n=1, k=p.k, N=p.N, level=CB_L, base_log=CB_B)
    want, _, _ = B.vertical_packing(vp, ggsw.reshape(-1), B.to_device(W.lut_layout(luts, t, p.N), DEV), r, m, batch)
    out = _filled(env, (batch + 1, nblk, p.big_n + 1))
    B.wop_pbs_crt(p, ring["fbsk"], ring["d_ksk"], ring["d_fpksk"], d_in, B.to_device(luts, DEV), moduli, PP_L, PP_B,
                  CB_L, CB_B, out=out)
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got = B.to_host(out)
    assert np.array_equal(got[:batch], B.to_host(want))
    assert (got[batch] == np.uint64(SENTINEL)).all()


# ---------------------------------------------------------------------------------------------------------
# the reference-named triples
# ---------------------------------------------------------------------------------------------------------
INPUTS, BITS, WITH_PADDING = 2, 3, 4


@pytest.fixture(scope="module")
def named(env):
    """Two inputs of 3 message bits under a padding bit, the LUTs in the reference-named layout [tau][max(2^t, N)],
    the CPU reference of the one lookup and the extension's result on the same inputs."""
    B, torch, k = env["B"], env["torch"], env["keys"]
    delta_log, t = 64 - WITH_PADDING, INPUTS * BITS
    msgs = [5, 3]
    cts = B.lwe_encrypt(k["glwe_sk"], np.array([v << delta_log for v in msgs], dtype=np.uint64), Cs.K * Cs.N,
                        Cs.INPUT_STD, 9971)
    rng = np.random.RandomState(9972)
    table = rng.randint(0, 1 << Cs.WIDTH, size=(INPUTS, 1 << t)).astype(np.uint64)
    luts = table << np.uint64(64 - Cs.WIDTH)
    padded = W.lut_layout(luts, t, Cs.N).reshape(INPUTS, Cs.N)
    bits = W.extract_bits(cts, k["bsk"], k["ksk"], [BITS] * INPUTS, [delta_log] * INPUTS, [0, BITS], Cs.OP)
    want = W.cbs_vp(bits[None], luts, k["bsk"], k["fpksk"], Cs.OP, Cs.PKSK, Cs.CBS)[0]
    d_cts = B.to_device(cts, DEV)
    d_bits = B.extract_bits(Cs.P, env["fbsk"], env["d_ksk"], d_cts, BITS, delta_log)
    ext, _ = B.circuit_bootstrap_vertical_packing(Cs.P, env["fbsk"], env["d_fpksk"], d_bits.reshape(1, t, Cs.LWE_N + 1),
                                                  B.to_device(luts, DEV), *Cs.PKSK, *Cs.CBS)
    torch.cuda.synchronize()
    ext = B.to_host(ext)[0]
    assert np.array_equal(ext, want), "the extension differs from the reference"
    index = (msgs[0] << BITS) | msgs[1]  # input 0 supplies the most significant bits
    assert Cs.messages(Cs.decrypt(want)) == [int(table[o, index]) for o in range(INPUTS)]
    return dict(d_cts=d_cts, d_bits=d_bits, d_padded=B.to_device(padded, DEV), ext=ext, delta_log=delta_log, t=t)


@pytest.mark.parametrize("with_buffer", (True, False), ids=("buffer", "null"))
def test_cuda_wop_pbs_64(env, named, with_buffer):
    L, B, torch = env["L"], env["B"], env["torch"]
    stream = B._stream(DEV)
    (bl, bb), (kl, kb), (pl, pb), (cl, cb) = Cs.BSK, Cs.KS, Cs.PKSK, Cs.CBS
    buf, dl, cdl = C.c_void_p(None), C.c_uint32(0), C.c_uint32(0)
    L.scratch_cuda_wop_pbs_64(stream, 0, C.byref(buf), C.byref(dl), C.byref(cdl), Cs.K, Cs.LWE_N, Cs.N, cl, bl,
                              WITH_PADDING, BITS, INPUTS, 0, with_buffer)
    assert bool(buf.value) == with_buffer
    assert (dl.value, cdl.value) == (named["delta_log"], 63)
    out = _filled(env, (INPUTS + 1, Cs.K * Cs.N + 1))
    L.cuda_wop_pbs_64(stream, 0, out.data_ptr(), named["d_cts"].data_ptr(), named["d_padded"].data_ptr(),
                      env["fbsk"].data_ptr(), env["d_ksk"].data_ptr(), env["d_fpksk"].data_ptr(), buf, cdl.value, Cs.K,
                      Cs.LWE_N, Cs.N, bb, bl, kb, kl, pb, pl, cb, cl, WITH_PADDING, BITS, dl.value, INPUTS, 0)
    L.cleanup_cuda_wop_pbs(stream, 0, C.byref(buf))
    assert not buf.value
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got = B.to_host(out)
    assert np.array_equal(got[:INPUTS], named["ext"])
    assert (got[INPUTS] == np.uint64(SENTINEL)).all()


@pytest.mark.parametrize("with_buffer", (True, False), ids=("buffer", "null"))
def test_cuda_circuit_bootstrap_vertical_packing_64(env, named, with_buffer):
    """The same lookup from the bit ciphertexts stage 1 left."""
    L, B, torch = env["L"], env["B"], env["torch"]
    stream = B._stream(DEV)
    (bl, bb), (pl, pb), (cl, cb) = Cs.BSK, Cs.PKSK, Cs.CBS
    buf, cdl = C.c_void_p(None), C.c_uint32(0)
    L.scratch_cuda_circuit_bootstrap_vertical_packing_64(stream, 0, C.byref(buf), C.byref(cdl), Cs.K, Cs.LWE_N, Cs.N,
                                                         cl, named["t"], INPUTS, 0, with_buffer)
    assert bool(buf.value) == with_buffer and cdl.value == 63
    out = _filled(env, (INPUTS + 1, Cs.K * Cs.N + 1))
    L.cuda_circuit_bootstrap_vertical_packing_64(stream, 0, out.data_ptr(), named["d_bits"].data_ptr(),
                                                 env["fbsk"].data_ptr(), env["d_fpksk"].data_ptr(),
                                                 named["d_padded"].data_ptr(), buf, cdl.value, Cs.N, Cs.K, Cs.LWE_N, bl,
                                                 bb, pl, pb, cl, cb, named["t"], INPUTS, 0)
    L.cleanup_cuda_circuit_bootstrap_vertical_packing(stream, 0, C.byref(buf))
    assert not buf.value
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got = B.to_host(out)
    assert np.array_equal(got[:INPUTS], named["ext"])
    assert (got[INPUTS] == np.uint64(SENTINEL)).all()


# ---------------------------------------------------------------------------------------------------------
# the memref routes
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keyset(env):
    k = env["keys"]
    ks = env["RT"].Keyset()
    ks.add_bsk(0, k["bsk"], Cs.P)
    ks.add_ksk(0, k["ksk"], Cs.P)
    ks.add_fpksk(0, k["fpksk"], Cs.P, *Cs.PKSK)
    yield ks
    ks.close()


@pytest.mark.parametrize("cuda_name", (False, True), ids=("hip_u64", "cuda_u64"))
@pytest.mark.parametrize("moduli", (Cs.MODULI_SETS[0], Cs.MODULI_SETS[2]), ids=IDS)
def test_memref_routes_equal_the_reference(env, keyset, moduli, cuda_name):
    """Host memrefs that start 5 words into their allocations, one value per call: value 0 through the keyset
    handle, value 1 through a bound runtime-context pointer."""
    RT = env["RT"]
    c = Cs.case(moduli)
    b = int(cuda_name)
    context = 0xC0FFEE00
    if cuda_name:
        keyset.bind(context)
    got = RT.wop_pbs_crt(context if cuda_name else keyset, Cs.P, c["blocks"][b], c["luts"], moduli, Cs.PKSK, Cs.CBS,
                         offset=5, cuda_name=cuda_name)
    assert np.array_equal(got, c["want"][b])


# ---------------------------------------------------------------------------------------------------------
# a gate refusal writes nothing
# ---------------------------------------------------------------------------------------------------------
def test_gate_refusal_leaves_the_output_untouched(env):
    """The bootstrapping key whose every word is 0x5555... at k = 1, N = 1024, level 1, base_log 11 (tests/
    test_gpu_circuit_bootstrap.py): the PBS exactness gate refuses it, so both chained calls return -2 and lwe_out
    keeps its sentinel."""
    L, B, torch = env["L"], env["B"], env["torch"]
    p = B.PbsParams(n=6, k=1, N=1024, level=1, base_log=11, ks_level=4, ks_base_log=3)
    fk = B.convert_bsk(p, np.full(p.bsk_len, 0x5555555555555555, dtype=np.uint64), DEV)
    torch.cuda.synchronize()
    assert L.concrete_hip_key_error_bound(fk.data_ptr(), p.base_log) >= 0.5
    (pl, pb), (cl, cb), moduli = (2, 15), (2, 8), (3, 4, 5)
    assert B.wop_pbs_supported(p, pl, pb, cl, cb)
    rng = np.random.RandomState(9980)
    d_fpksk = B.to_device(_rand_u64(rng, B.fpksk_words(p.k, p.N, pl)), DEV)
    d_ksk = B.to_device(_rand_u64(rng, p.ksk_len), DEV)
    d_in = B.to_device(_rand_u64(rng, (2, len(moduli), p.lwe_out_size)), DEV)
    d_bits = B.to_device(_rand_u64(rng, (2, 7, p.n + 1)), DEV)
    d_luts = B.to_device(_rand_u64(rng, (len(moduli), 1 << 7)), DEV)
    mods = np.array(moduli, dtype=np.uint64)
    out = _filled(env, (2, len(moduli), p.lwe_out_size))
    rc = L.concrete_hip_wop_pbs_crt(B._stream(DEV), 0, out.data_ptr(), d_in.data_ptr(), d_luts.data_ptr(), fk.data_ptr(),
                                    d_ksk.data_ptr(), d_fpksk.data_ptr(), mods.ctypes.data, len(moduli), 2, p.n, p.k,
                                    p.N, p.level, p.base_log, p.ks_level, p.ks_base_log, pl, pb, cl, cb, None, 0, None)
    torch.cuda.synchronize()
    assert rc == -2, L.concrete_hip_last_error()
    assert b"certified rounding bound" in L.concrete_hip_last_error()
    assert (B.to_host(out) == np.uint64(SENTINEL)).all()
    rc = L.concrete_hip_circuit_bootstrap_vertical_packing(B._stream(DEV), 0, out.data_ptr(), d_bits.data_ptr(),
                                                           d_luts.data_ptr(), fk.data_ptr(), d_fpksk.data_ptr(), p.n,
                                                           p.k, p.N, p.level, p.base_log, pl, pb, cl, cb, 7,
                                                           len(moduli), 2, None, 0, None)
    torch.cuda.synchronize()
    assert rc == -2, L.concrete_hip_last_error()
    assert (B.to_host(out) == np.uint64(SENTINEL)).all()
    assert B.stream_status(DEV) == 0
