"""GPU tests of the circuit bootstrap (WoP-PBS stage 2) and its private functional packing keyswitch
(concrete_amd/csrc/circuit_bootstrap.hip).

The definition is tests/cbs_reference.py: the oracle's integer PBS and the oracle's LWE keyswitch on zero-padded
rows.  The device computes the same integers, so every comparison here is word for word; there is no tolerance
anywhere.  Outputs are sentinel-filled before each call and carry one GLWE (or row) more than the call writes,
which must keep the sentinel.  References are computed once per (shape, decomposition) for the largest row
count and sliced: rows are independent, and a level matrix depends on its own level only.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cbs_reference as R  # noqa: E402
import table_shapes as S  # noqa: E402
import vp_reference as V  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY_STD = 2.0 ** -52
SENTINEL = 0x5A5A5A5A5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry():
    """The fp-ks kernel's tile constants, from its header: (rows per workgroup, columns per workgroup, workgroups
    aimed for, fewest blocks per split)."""
    txt = open(os.path.join(ROOT, "concrete_amd", "csrc", "circuit_bootstrap.hpp")).read()
    get = lambda name: int(re.search(r"\b%s = (\d+);" % name, txt).group(1))  # noqa: E731
    return get("FPKS_ROWS"), get("FPKS_THREADS"), get("FPKS_TARGET_WGS"), get("FPKS_MIN_BLOCKS")


T, COLS, TARGET_WGS, MIN_BLOCKS = _geometry()


def _splits(k, N, rows):
    """circuit_bootstrap.hip:fpks_splits."""
    wgs = -(-((k + 1) * N) // COLS) * -(-rows // T)
    return max(1, min(-(-TARGET_WGS // wgs), max(1, (k * N + 1) // MIN_BLOCKS)))


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from concrete_amd import _native
    from concrete_amd import backend as B
    from oracle import pyoracle as O
    O.lib()
    return dict(torch=torch, L=_native.lib(), B=B, O=O, N=_native, fpks={}, cbs={}, keys={})


def _rand_u64(rng, shape):
    return rng.randint(0, 1 << 32, size=shape).astype(np.uint64) << np.uint64(32) | \
        rng.randint(0, 1 << 32, size=shape).astype(np.uint64)


def _filled(env, shape):
    t = env["torch"].empty(shape, dtype=env["torch"].int64, device=DEV)
    t.fill_(SENTINEL)  # below 2^63: the same bits as int64
    return t


# ---------------------------------------------------------------------------------------------------------
# fp-ks
# ---------------------------------------------------------------------------------------------------------
FPKS_SHAPES = [(1, 256), (2, 512)]
FPKS_DECOMP = [(1, 25), (2, 15), (3, 13), (4, 10), (2, 31), (1, 40)]  # the last: a digit beyond 32 bits
# and the WoP table's seven (pp_l, pp_b), up to 8 levels: (4, 10) is in the list above already
FPKS_DECOMP += [d for d in S.WOP_PP if d not in FPKS_DECOMP]
ROW_COUNTS = (1, 2, T - 1, T, T + 1, 2 * T + 1)
MAX_ROWS = 2 * T + 1


def _fpks_case(env, k, N, level, base_log, keys=None, max_rows=MAX_ROWS):
    """Random key words (the map is linear: any words pin it), random rows with the decomposition's edge values
    in row 0 and 1, the reference for max_rows rows and `keys` (k + 1 unless given) keys, and the key on the device."""
    keys = k + 1 if keys is None else keys
    key = (k, N, level, base_log, keys, max_rows)
    if key in env["fpks"]:
        return env["fpks"][key]
    B = env["B"]
    rng = np.random.RandomState(9400 + 1000 * k + N + 17 * level + base_log)
    W, G = k * N + 1, (k + 1) * N
    fpksk = _rand_u64(rng, (keys, W, level, G))
    rows = _rand_u64(rng, (max_rows, W))
    nrep = 64 - level * base_log
    q = _rand_u64(rng, 8) >> np.uint64(nrep)
    half_step = (q << np.uint64(nrep)) | np.uint64(1 << (nrep - 1))  # the dropped bits are exactly half a step
    rows[0, :4] = [np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1 << 63), half_step[0], half_step[1]]
    rows[0, W - 1] = half_step[2]                                    # the body is decomposed like any word
    rows[0, W - 2] = np.uint64((1 << 63) - 1)
    rows[1, :4] = [half_step[3], np.uint64(0), np.uint64(1 << (nrep - 1)), half_step[4]]
    rows[1, W - 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    want = R.fp_keyswitch(rows, fpksk, k, N, level, base_log)
    for a in (fpksk, rows, want):
        a.setflags(write=False)
    c = dict(fpksk=fpksk, rows=rows, want=want, d_key=B.to_device(fpksk.reshape(-1).copy(), DEV))
    env["fpks"] = {key: c}  # one key on the device at a time
    return c


@pytest.mark.parametrize("decomp", FPKS_DECOMP, ids=lambda d: f"l{d[0]}b{d[1]}")
@pytest.mark.parametrize("shape", FPKS_SHAPES, ids=lambda s: f"k{s[0]}N{s[1]}")
def test_fp_keyswitch_bit_exact(env, shape, decomp):
    B, torch = env["B"], env["torch"]
    (k, N), (level, base_log) = shape, decomp
    c = _fpks_case(env, k, N, level, base_log)
    G = (k + 1) * N
    assert {_splits(k, N, r) > 1 for r in ROW_COUNTS} == {True}  # these counts all split; the unsplit one is below
    for rows in ROW_COUNTS:
        d_in = B.to_device(c["rows"][:rows].copy(), DEV)
        for nk in (1, k + 1):
            out = _filled(env, (rows + 1, nk, G))  # one GLWE row more than the call writes
            B.fp_keyswitch(k, N, level, base_log, c["d_key"], d_in, num_keys=nk, out=out)
            torch.cuda.synchronize()
            got = B.to_host(out)
            assert np.array_equal(got[:rows], c["want"][:rows, :nk]), f"{rows} rows, {nk} keys"
            assert (got[rows] == np.uint64(SENTINEL)).all(), f"{rows} rows, {nk} keys: wrote past the output"


@pytest.mark.parametrize("decomp", S.WOP_PP, ids=lambda d: f"l{d[0]}b{d[1]}")
def test_fp_keyswitch_at_the_table_ring(env, decomp):
    """The WoP table's own ring (k = 2, N = 1024: 2049 blocks, 3072 output words) at each of its (pp_l, pp_b), one
    key of random words (403 MB at 8 levels), one row and one row more than a workgroup's tile."""
    B, torch = env["B"], env["torch"]
    (k, N), (level, base_log) = S.WOP_RING, decomp
    counts = (1, T + 1)
    c = _fpks_case(env, k, N, level, base_log, keys=1, max_rows=max(counts))
    G = (k + 1) * N
    for rows in counts:
        out = _filled(env, (rows + 1, 1, G))  # one GLWE row more than the call writes
        B.fp_keyswitch(k, N, level, base_log, c["d_key"], B.to_device(c["rows"][:rows].copy(), DEV), num_keys=1, out=out)
        torch.cuda.synchronize()
        got = B.to_host(out)
        assert np.array_equal(got[:rows], c["want"][:rows]), f"{rows} rows"
        assert (got[rows] == np.uint64(SENTINEL)).all(), f"{rows} rows: wrote past the output"


def test_fp_keyswitch_unsplit_row_count(env):
    """Enough rows that the column windows and row tiles alone fill the chip: the (block, level) axis is not
    split (every other case here splits it).  k = 1, N = 256, one key, level 1."""
    B, torch = env["B"], env["torch"]
    k, N, level, base_log = 1, 256, 1, 25
    rows = T * -(-TARGET_WGS // (-(-((k + 1) * N) // COLS)))
    assert _splits(k, N, rows) == 1 and _splits(k, N, rows - T) > 1
    rng = np.random.RandomState(9490)
    fpksk = _rand_u64(rng, (1, k * N + 1, level, (k + 1) * N))
    lwe = _rand_u64(rng, (rows, k * N + 1))
    want = R.fp_keyswitch(lwe, fpksk, k, N, level, base_log)
    out = _filled(env, (rows + 1, 1, (k + 1) * N))
    B.fp_keyswitch(k, N, level, base_log, B.to_device(fpksk.reshape(-1), DEV), B.to_device(lwe, DEV), num_keys=1, out=out)
    torch.cuda.synchronize()
    got = B.to_host(out)
    assert np.array_equal(got[:rows], want)
    assert (got[rows] == np.uint64(SENTINEL)).all()


@pytest.mark.parametrize("shape", FPKS_SHAPES, ids=lambda s: f"k{s[0]}N{s[1]}")
def test_reference_named_fp_keyswitch_wraps_the_keys(env, shape):
    """cuda_fp_keyswitch_lwe_to_glwe_64 on 2 (k+1) + 1 rows: row i goes through key i mod (k+1) into GLWE i."""
    L, B, torch = env["L"], env["B"], env["torch"]
    k, N = shape
    level, base_log = 2, 15
    c = _fpks_case(env, k, N, level, base_log)
    rows, nk, G = 2 * (k + 1) + 1, k + 1, (k + 1) * N
    out = _filled(env, (rows + 1, G))
    d_in = B.to_device(c["rows"][:rows].copy(), DEV)
    L.cuda_fp_keyswitch_lwe_to_glwe_64(B._stream(DEV), 0, out.data_ptr(), d_in.data_ptr(), c["d_key"].data_ptr(), k * N,
                                       k, N, base_log, level, rows, nk)
    torch.cuda.synchronize()
    got = B.to_host(out)
    want = np.stack([c["want"][i, i % nk] for i in range(rows)])
    assert np.array_equal(got[:rows], want)
    assert (got[rows] == np.uint64(SENTINEL)).all()


# ---------------------------------------------------------------------------------------------------------
# circuit bootstrap
# ---------------------------------------------------------------------------------------------------------
# (k, N, n), BSK (level, base_log), fp-ks key (level, base_log), base_log_cbs, real fp-ks key or random words
CBS_SHAPES = {
    "n512": ((1, 512, 8), (2, 10), (2, 15), 10, True),      # the general path
    "n1024": ((1, 1024, 8), (3, 7), (3, 13), 8, True),      # a hand-tuned kernel (the pair kernel)
    "k2n1024": ((2, 1024, 8), (2, 15), (2, 17), 8, False),  # the WoP table's ring, 15-bit PBS digits, 3 keys
}
MAX_LEVEL_CBS, MAX_SAMPLES = 4, 5
# (level_cbs, samples, delta_log): every value of each at every shape
CBS_RUNS = [(1, 1, 63), (2, 3, 59), (4, 5, 63), (4, 1, 59), (2, 5, 63), (1, 3, 59)]


def _cbs_keys(env, shape, pp=None):
    """Secret keys, the standard and the device BSK and the fp-ks key list of a shape, at the shape's own fp-ks
    decomposition or at pp = (level, base_log); kept until another (shape, pp) is asked for."""
    if (shape, pp) in env["keys"]:
        return env["keys"][(shape, pp)]
    B, O = env["B"], env["O"]
    (k, N, n), (bl, bb), (pl, pb), _, real = CBS_SHAPES[shape]
    pl, pb = pp or (pl, pb)
    seed = 9500 + 10 * sorted(CBS_SHAPES).index(shape)
    p = B.PbsParams(n=n, k=k, N=N, level=bl, base_log=bb)
    lwe_sk, glwe_sk = B.binary_key(n, seed), B.binary_key(k * N, seed + 1)
    bsk = B.bsk_generate(p, lwe_sk, glwe_sk, seed + 2, std=KEY_STD)
    if real:
        fpksk = B.fpksk_generate(p, glwe_sk, pl, pb, seed + 3, std=KEY_STD)
    else:
        fpksk = _rand_u64(np.random.RandomState(seed + 3), (k + 1, k * N + 1, pl, (k + 1) * N))
    e = dict(p=p, lwe_sk=lwe_sk, glwe_sk=glwe_sk, bsk=bsk, fpksk=fpksk, fbsk=B.convert_bsk(p, bsk, DEV),
             d_fpksk=B.to_device(fpksk.reshape(-1), DEV))
    env["keys"] = {(shape, pp): e}  # one shape's keys on the device at a time
    return e


def _cbs_case(env, shape, delta_log):
    """MAX_SAMPLES encrypted bits at delta_log and the reference at MAX_LEVEL_CBS levels: fewer samples are a prefix,
    fewer levels the first level matrices (level matrix v depends on v and base_log_cbs only)."""
    key = (shape, delta_log)
    if key in env["cbs"]:
        return env["cbs"][key]
    B = env["B"]
    e = _cbs_keys(env, shape)
    (k, N, n), (bl, bb), (pl, pb), cb, _ = CBS_SHAPES[shape]
    bits = [1, 0, 1, 1, 0][:MAX_SAMPLES]
    cts = B.lwe_encrypt(e["lwe_sk"], [b << delta_log for b in bits], n, KEY_STD, 9600 + delta_log)
    ggsw, w = R.circuit_bootstrap(cts, e["bsk"], e["fpksk"], delta_log, n, k, N, bl, bb, pl, pb, MAX_LEVEL_CBS, cb)
    for a in (cts, ggsw, w):
        a.setflags(write=False)
    c = dict(cts=cts, ggsw=ggsw, w=w, bits=bits)
    env["cbs"][key] = c
    return c


@pytest.mark.parametrize("run", CBS_RUNS, ids=lambda r: f"l{r[0]}s{r[1]}d{r[2]}")
@pytest.mark.parametrize("shape", sorted(CBS_SHAPES))
def test_circuit_bootstrap_bit_exact(env, shape, run):
    level_cbs, samples, delta_log = run
    _, _, (pl, pb), cb, _ = CBS_SHAPES[shape]
    e = _cbs_keys(env, shape)
    c = _cbs_case(env, shape, delta_log)
    _run_and_compare(env, e, c["cts"][:samples], delta_log, (pl, pb), (level_cbs, cb), c["ggsw"][:samples, :level_cbs],
                     c["w"][:samples, :level_cbs], own_scratch=samples == 3)


def _run_and_compare(env, e, cts, delta_log, pp, cbs, want_ggsw, want_w, own_scratch=False):
    """One circuit bootstrap of the rows `cts` with the keys `e`: the rows after the PBS and the GGSWs equal the
    reference, the GLWE and the row past the call's output keep the sentinel, the stream's status is clean."""
    B, torch = env["B"], env["torch"]
    p, samples, (pl, pb), (level_cbs, cb) = e["p"], cts.shape[0], pp, cbs
    k, N = p.k, p.N
    assert B.circuit_bootstrap_supported(p, pl, pb, level_cbs, cb)
    out = _filled(env, (samples + 1, level_cbs, k + 1, (k + 1) * N))
    w = _filled(env, (samples + 1, level_cbs, k * N + 1))
    scratch = None
    if own_scratch:  # the caller's scratch, exactly the size the query names; elsewhere the pool's
        need = B.circuit_bootstrap_scratch_bytes(p, level_cbs, samples)
        assert need > 0 and need % 16 == 0
        scratch = torch.empty(need // 8, dtype=torch.int64, device=DEV)
    B.circuit_bootstrap(p, e["fbsk"], e["d_fpksk"], B.to_device(cts.copy(), DEV), delta_log, pl, pb, level_cbs, cb,
                        out=out, scratch=scratch, pbs_out=w)
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    got_w, got = B.to_host(w), B.to_host(out)
    assert np.array_equal(got_w[:samples], want_w), "the rows after the PBS differ (before the fp-ks)"
    assert np.array_equal(got[:samples], want_ggsw), "the GGSWs differ (in the fp-ks)"
    sentinel = np.uint64(SENTINEL)
    assert (got_w[samples] == sentinel).all() and (got[samples] == sentinel).all(), "wrote past the output"


# The WoP table's 32 distinct (cb_l, cb_b, pp_l, pp_b), ordered by (pp, cb) so that one fp-ks key serves its run of
# pairs: all of them on n512 with a real fp-ks key, those of at most 2 fp-ks levels (a key list of <= 302 MB) on
# the table's own ring with random key words.  Each runs at level_cbs = cb_l (up to 32; CBS_RUNS stop at 4).
CBS_TABLE_PAIRS = sorted(S.distinct(S.WOP_ROWS, "cb_l", "cb_b", "pp_l", "pp_b"), key=lambda q: (q[2:], q[:2]))
CBS_TABLE_CASES = [("n512", q) for q in CBS_TABLE_PAIRS] + [("k2n1024", q) for q in CBS_TABLE_PAIRS if q[2] <= 2]


@pytest.mark.parametrize("case", CBS_TABLE_CASES, ids=lambda c: "%s-cb%d_%d-pp%d_%d" % ((c[0],) + c[1]))
def test_circuit_bootstrap_table_pairs(env, case):
    B = env["B"]
    shape, (cb_l, cb_b, pl, pb) = case
    (k, N, n), (bl, bb), _, _, _ = CBS_SHAPES[shape]
    e = _cbs_keys(env, shape, pp=(pl, pb))
    delta_log = (63, 59)[CBS_TABLE_PAIRS.index(case[1]) % 2]
    cts = B.lwe_encrypt(e["lwe_sk"], [b << delta_log for b in (1, 0)], n, KEY_STD, 9650 + delta_log)
    ggsw, w = R.circuit_bootstrap(cts, e["bsk"], e["fpksk"], delta_log, n, k, N, bl, bb, pl, pb, cb_l, cb_b)
    _run_and_compare(env, e, cts, delta_log, (pl, pb), (cb_l, cb_b), ggsw, w)


@pytest.mark.parametrize("with_buffer", (True, False), ids=("buffer", "null"))
def test_reference_named_calls_equal_the_extension(env, with_buffer):
    """scratch_cuda_circuit_bootstrap_64 / cuda_circuit_bootstrap_64 / cleanup_cuda_circuit_bootstrap with a
    buffer from the scratch call and with NULL (pool scratch); lut_vector_indexes NULL and written out."""
    L, B, torch = env["L"], env["B"], env["torch"]
    shape, level_cbs, samples, delta_log = "n512", 2, 3, 63
    (k, N, n), (bl, bb), (pl, pb), cb, _ = CBS_SHAPES[shape]
    e = _cbs_keys(env, shape)
    c = _cbs_case(env, shape, delta_log)
    stream = B._stream(DEV)
    d_in = B.to_device(c["cts"][:samples].copy(), DEV)
    idx = B.to_device(np.tile(np.arange(level_cbs, dtype=np.uint64), samples), DEV) if with_buffer else None
    out = _filled(env, (samples + 1, level_cbs, k + 1, (k + 1) * N))
    buf = C.c_void_p(None)
    L.scratch_cuda_circuit_bootstrap_64(stream, 0, C.byref(buf), k, n, N, level_cbs, samples, 0, with_buffer)
    assert bool(buf.value) == with_buffer
    L.cuda_circuit_bootstrap_64(stream, 0, out.data_ptr(), d_in.data_ptr(), e["fbsk"].data_ptr(), e["d_fpksk"].data_ptr(),
                                None if idx is None else idx.data_ptr(), buf, delta_log, N, k, n, bl, bb, pl, pb,
                                level_cbs, cb, samples, 0)
    L.cleanup_cuda_circuit_bootstrap(stream, 0, C.byref(buf))
    assert not buf.value
    ext = B.circuit_bootstrap(e["p"], e["fbsk"], e["d_fpksk"], d_in, delta_log, pl, pb, level_cbs, cb)
    torch.cuda.synchronize()
    got = B.to_host(out)
    assert np.array_equal(got[:samples], B.to_host(ext))
    assert np.array_equal(got[:samples], c["ggsw"][:samples, :level_cbs])
    assert (got[samples] == np.uint64(SENTINEL)).all()


def test_end_to_end_with_vertical_packing(env):
    """Real keys from concrete_hip_fpksk_generate, 6 encrypted bits, circuit bootstrap, then
    concrete_hip_vertical_packing (r = 3, m = 3, tau = 2) on LUTs of 2-bit messages: the outputs decrypt to the
    table entry the bits select, and vp_reference on the same GGSWs gives the same words.
    The circuit bootstrap here is (level 4, base_log 5).  Every GGSW message carries the rounding error of its PBS,
    about 2^48 at BSK (2, 10) whatever the message's size, and a CMUX multiplies it by digits of up to
    2^(base_log_cbs - 1) over (k+1) N level_cbs terms: at base_log_cbs 10 six CMUXes drift by 2^61 to 2^62 on the
    CPU reference, past the 2^61 half-window of a 2-bit message, at base_log_cbs 5 by 2^57, four bits inside it."""
    B, O, torch = env["B"], env["O"], env["torch"]
    shape = "n512"
    (k, N, n), (bl, bb), (pl, pb), _, real = CBS_SHAPES[shape]
    assert real
    e = _cbs_keys(env, shape)
    level_cbs, cb, r, m, tau, width = 4, 5, 3, 3, 2, 2
    bits = [1, 0, 1, 0, 1, 1]
    cts = B.lwe_encrypt(e["lwe_sk"], [b << 63 for b in bits], n, KEY_STD, 9700)
    ggsw = B.circuit_bootstrap(e["p"], e["fbsk"], e["d_fpksk"], B.to_device(cts, DEV), 63, pl, pb, level_cbs, cb)
    rng = np.random.RandomState(9701)
    table = rng.randint(0, 1 << width, size=(tau, 1 << r, N)).astype(np.uint64)
    luts = table << np.uint64(64 - width)
    vp = B.PbsParams(n=1, k=k, N=N, level=level_cbs, base_log=cb)
    assert B.vertical_packing_supported(vp)
    lwe, _, _ = B.vertical_packing(vp, ggsw.reshape(-1), B.to_device(luts, DEV), r, m, 1)
    torch.cuda.synchronize()
    assert B.stream_status(DEV) == 0
    lwe = B.to_host(lwe)
    pi, ci = V.selected(luts, bits[:r], bits[r:])
    dec = O.lwe_decrypt_batch(e["glwe_sk"], np.ascontiguousarray(lwe[0]), k * N)
    got = [((int(d) + (1 << (63 - width))) >> (64 - width)) % (1 << width) for d in dec]
    assert got == [int(table[o, pi, ci]) for o in range(tau)]
    host = B.to_host(ggsw).reshape(1, r + m, level_cbs, k + 1, k + 1, N)
    want, _ = V.vertical_packing(host, luts, r, m, k, N, level_cbs, cb)
    assert np.array_equal(lwe, want)


def test_gate_refuses_a_key_with_a_large_spectrum(env):
    """A bootstrapping key whose every word is 0x5555... at k = 1, N = 1024, level 1, base_log 11: the PBS
    exactness gate refuses it (tests/test_gpu_robustness.py), so the circuit bootstrap returns -2 and writes
    nothing."""
    L, B, torch = env["L"], env["B"], env["torch"]
    p = B.PbsParams(n=6, k=1, N=1024, level=1, base_log=11)
    fk = B.convert_bsk(p, np.full(p.bsk_len, 0x5555555555555555, dtype=np.uint64), DEV)
    torch.cuda.synchronize()
    assert L.concrete_hip_key_error_bound(fk.data_ptr(), p.base_log) >= 0.5
    pl, pb, level_cbs, cb, samples = 2, 15, 2, 8, 2
    assert B.circuit_bootstrap_supported(p, pl, pb, level_cbs, cb)
    rng = np.random.RandomState(9800)
    d_key = B.to_device(_rand_u64(rng, R.fpksk_words(p.k, p.N, pl)), DEV)
    d_in = B.to_device(_rand_u64(rng, (samples, p.n + 1)), DEV)
    out = _filled(env, (samples, level_cbs, p.k + 1, p.glwe_size))
    w = _filled(env, (samples, level_cbs, p.lwe_out_size))
    rc = L.concrete_hip_circuit_bootstrap(B._stream(DEV), 0, out.data_ptr(), d_in.data_ptr(), fk.data_ptr(),
                                          d_key.data_ptr(), 63, p.n, p.k, p.N, p.level, p.base_log, pl, pb, level_cbs,
                                          cb, samples, None, 0, w.data_ptr())
    torch.cuda.synchronize()
    assert rc == -2, L.concrete_hip_last_error()
    assert b"certified rounding bound" in L.concrete_hip_last_error()
    sentinel = np.uint64(SENTINEL)
    assert (B.to_host(out) == sentinel).all() and (B.to_host(w) == sentinel).all()
