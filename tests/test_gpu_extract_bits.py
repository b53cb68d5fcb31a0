"""GPU tests of the batched LWE bit extraction (WoP-PBS stage 1; concrete_amd/csrc/extract_bits.hip,
DESIGN.md §4.15).

Per input ciphertext c (dimension kN), nb = number_of_bits, dl = delta_log, wrapping u64:

    c' = c
    for t = 0 .. nb-1:
        u = KS(c' << (64 - dl - t - 1));  out[nb-1-t] = u;  stop after the last bit
        u.body += 2^62;  v = PBS(u, acc);  acc = trivial GLWE, every body coefficient -(2^(dl-1+t))
        v.body += 2^(dl-1+t);  c' -= v

The keyswitch and the PBS are exact and deterministic, so the fused call is checked word for word: against
this loop run on the CPU oracle's exact (integer) mode, and against the loop composed from the GPU's own
public keyswitch and PBS.  Keys are near-noiseless (sigma 2^-52) at reduced n, as in
tests/test_gpu_robustness.py; the bit-exact checks do not depend on the noise, the decrypt checks keep
every phase well inside its window.  out[j] encrypts bit j (most significant first) times 2^63, the bits
being those of ((pt + 2^(dl-1)) >> dl) mod 2^nb; a decrypted phase is read by rounding to the nearest
multiple of 2^63.
"""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY_STD = 2.0 ** -52
M64 = (1 << 64) - 1
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from concrete_amd import _native
    from concrete_amd import backend as B
    from oracle import pyoracle as O
    return dict(torch=torch, L=_native.lib(), B=B, O=O, N=_native, setups={})


# Three rows of the optimizer's WoP table (tests/golden/wop_pbs_last_128_rows.json; k = 2, N = 1024), each with
# its own BSK and keyswitch decomposition, n cut to 8: name -> (bits, log_norm2, br_l, br_b, ks_l, ks_b).
# tests/test_keygen_abi.py holds them to the table.
WOP_ROWS = {
    "wop_fewest_bsk_levels": (1, 0, 2, 15, 3, 3),       # the fewest BSK levels of the table
    "wop_most_bsk_levels": (2, 20, 45, 1, 13, 1),       # the most
    "wop_deepest_keyswitch": (10, 14, 22, 2, 15, 1),    # the most keyswitch levels of the table
}
NAMES = ["cfg2", "cfg4", "opt1", "cfg2_full"] + list(WOP_ROWS)


def _shape(B, name):
    if name in WOP_ROWS:
        _, _, br_l, br_b, ks_l, ks_b = WOP_ROWS[name]
        return B.PbsParams(n=8, k=2, N=1024, level=br_l, base_log=br_b, ks_level=ks_l, ks_base_log=ks_b)
    return {"cfg2": replace(B.CFG2, n=8), "cfg4": replace(B.CFG4, n=8), "opt1": replace(B.OPTIMIZER_SETS[1], n=8),
            "cfg2_full": B.CFG2}[name]


def _setup(env, name):
    """Keys of one shape, generated once per module: secret keys, standard BSK / KSK on the host, the device
    Fourier key and the KSK on the device."""
    if name in env["setups"]:
        return env["setups"][name]
    B, O, torch = env["B"], env["O"], env["torch"]
    p = _shape(B, name)
    seed = 7100 + 10 * sorted(NAMES).index(name)
    lwe_sk = B.binary_key(p.n, seed)
    glwe_sk = B.binary_key(p.big_n, seed + 1)
    bsk = B.bsk_generate(p, lwe_sk, glwe_sk, seed + 2, std=KEY_STD)
    ksk = B.ksk_generate(p, glwe_sk, lwe_sk, seed + 3, std=KEY_STD)
    fbsk = B.convert_bsk(p, bsk, DEV)
    ksk_dev = B.to_device(ksk, DEV)
    torch.cuda.synchronize()
    op = O.Params(n=p.n, k=p.k, N=p.N, l=p.level, logB=p.base_log, ks_l=p.ks_level, ks_logB=p.ks_base_log)
    S = dict(p=p, op=op, lwe_sk=lwe_sk, glwe_sk=glwe_sk, bsk=bsk, ksk=ksk, fbsk=fbsk, ksk_dev=ksk_dev)
    env["setups"][name] = S
    return S


def _plaintexts(rng, nbs, dls):
    """Random plaintexts whose low dl bits stay at least 2^(dl-4) away from the rounding boundary 2^(dl-1);
    the bits above dl + nb are random too (the extraction must ignore them)."""
    pts = []
    for nb, dl in zip(nbs, dls):
        half, gap = 1 << (dl - 1), 1 << max(dl - 4, 0)
        low = int(rng.randint(0, 1 << 30)) * (1 << dl) >> 30
        if abs(low - half) < gap:
            low = (low + 2 * gap) % (1 << dl)
        assert abs(low - half) >= gap and 0 <= low < (1 << dl)
        hi = int(rng.randint(0, 1 << 30)) << 34 | int(rng.randint(0, 1 << 30))
        pts.append(((hi << dl) | low) & M64)
    return pts


def _expected_bits(pt, nb, dl):
    r = (((pt + (1 << (dl - 1))) & M64) >> dl) % (1 << nb)
    return [(r >> (nb - 1 - j)) & 1 for j in range(nb)]


def _encrypt_big(env, S, pts, seed):
    """Input ciphertexts under the big (GLWE-derived) key, dimension kN, noise 2^-25."""
    B, p = env["B"], S["p"]
    return B.lwe_encrypt(S["glwe_sk"], np.array(pts, dtype=np.uint64), p.big_n, 2.0 ** -25, seed)


def _const_acc(p, e):
    acc = np.zeros(p.glwe_size, dtype=np.uint64)
    acc[p.k * p.N:] = np.uint64((-(1 << e)) & M64)
    return acc


def _first_rows(nbs, offs):
    return np.concatenate([[0], np.cumsum(nbs)[:-1]]).astype(np.int64) if offs is None else np.asarray(offs, np.int64)


def _oracle_extract(env, S, cts, nbs, dls, offs=None):
    """The loop of the module docstring on the CPU: oracle keyswitch and PBS (schoolbook/Karatsuba integer
    mode: exact for every shape), numpy u64 arithmetic in between."""
    O, p, op = env["O"], S["p"], S["op"]
    nbs, dls = np.asarray(nbs, np.int64), np.asarray(dls, np.int64)
    first = _first_rows(nbs, offs)
    out = np.zeros((int(nbs.sum()), p.n + 1), dtype=np.uint64)
    c = cts.copy()
    for t in range(int(nbs.max())):
        act = np.nonzero(nbs > t)[0]
        sh = (64 - dls[act] - t - 1).astype(np.uint64)
        u = O.keyswitch_batch(op, c[act] << sh[:, None], S["ksk"])
        out[first[act] + nbs[act] - 1 - t] = u
        go = nbs[act] > t + 1
        if not go.any():
            break
        rows, u = act[go], u[go].copy()
        u[:, -1] += np.uint64(1 << 62)
        exps = (dls[rows] - 1 + t).astype(np.int64)
        uniq = sorted(set(exps.tolist()))
        luts = np.stack([_const_acc(p, e) for e in uniq])
        lut_idx = np.array([uniq.index(e) for e in exps.tolist()], dtype=np.uint64)
        v, _ = O.pbs_batch(op, u, luts, bsk=S["bsk"], lut_idx=lut_idx, mode=O.MODE_KARATSUBA)
        v[:, -1] += np.uint64(1) << exps.astype(np.uint64)
        c[rows] -= v
    return out


def _gpu_composition(env, S, d_in, nbs, dls):
    """The same loop from the GPU's public keyswitch and PBS with torch integer steps (packed output)."""
    B, torch, p = env["B"], env["torch"], S["p"]
    nbs_t = torch.tensor(nbs, dtype=torch.int64, device=DEV)
    dls_t = torch.tensor(dls, dtype=torch.int64, device=DEV)
    first = torch.tensor(_first_rows(np.asarray(nbs), None), dtype=torch.int64, device=DEV)
    out = torch.zeros((int(sum(nbs)), p.n + 1), dtype=torch.int64, device=DEV)
    exps_all = sorted({dl - 1 + t for nb, dl in zip(nbs, dls) for t in range(nb - 1)})
    accs = B.to_device(np.stack([_const_acc(p, e) for e in exps_all]), DEV) if exps_all else None
    slot = torch.full((64,), -1, dtype=torch.int64, device=DEV)
    for i, e in enumerate(exps_all):
        slot[e] = i
    c = d_in.clone()
    for t in range(max(nbs)):
        act = torch.nonzero(nbs_t > t)[:, 0]
        s = torch.bitwise_left_shift(c[act], (64 - dls_t[act] - t - 1)[:, None]).contiguous()
        u = B.keyswitch(p, S["ksk_dev"], s)
        out[first[act] + nbs_t[act] - 1 - t] = u
        go = nbs_t[act] > t + 1
        if not bool(go.any()):
            break
        rows, u = act[go], u[go].contiguous()
        u[:, -1] += 1 << 62
        exps = dls_t[rows] - 1 + t
        v = B.pbs(p, S["fbsk"], u, accs, lut_idx=slot[exps].contiguous())
        v[:, -1] += torch.bitwise_left_shift(torch.ones_like(exps), exps)
        c[rows] -= v
    return out


def _decrypt_bits(env, S, out_words):
    """Each output row's phase under the small key, rounded to the nearest multiple of 2^63."""
    B, p = env["B"], S["p"]
    dec = B.lwe_decrypt(S["lwe_sk"], out_words, p.n)
    return [((int(d) + (1 << 62)) >> 63) & 1 for d in dec]


# ------------------------------------------------------------------------------------------------
# 1. bit-exact against the oracle composition: the N = 1024 and N = 2048 kernels, a k > 1 shape, and three
#    rows of the WoP table at its own ring
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2", "cfg4", "opt1"] + list(WOP_ROWS))
def test_bit_exact_against_oracle(env, name):
    B, torch = env["B"], env["torch"]
    S = _setup(env, name)
    rows, nb, dl = 5, 4, 60
    rng = np.random.RandomState(11)
    pts = _plaintexts(rng, [nb] * rows, [dl] * rows)
    cts = _encrypt_big(env, S, pts, 7201)
    got = B.to_host(B.extract_bits(S["p"], S["fbsk"], S["ksk_dev"], B.to_device(cts, DEV), nb, dl))
    assert B.stream_status(DEV) == 0
    ref = _oracle_extract(env, S, cts, [nb] * rows, [dl] * rows)
    assert got.shape == ref.shape == (rows * nb, S["p"].n + 1)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {got.size} output words differ from the oracle"
    bits = _decrypt_bits(env, S, got)
    assert bits == [b for pt in pts for b in _expected_bits(pt, nb, dl)]


# ------------------------------------------------------------------------------------------------
# 2. heterogeneous rows, permuted output blocks, caller-visible scratch
# ------------------------------------------------------------------------------------------------
def test_heterogeneous_rows_and_output_offsets(env):
    B, torch = env["B"], env["torch"]
    S = _setup(env, "cfg2")
    p = S["p"]
    nbs = [1, 3, 5, 2, 3]
    dls = [63, 61, 59, 59, 61]  # 64 - nb, except row 3: nb = 2 at dl = 59 leaves three bits above unread
    total = sum(nbs)
    # the blocks in the order 2, 0, 4, 3, 1
    offs = np.zeros(len(nbs), dtype=np.uint64)
    at = 0
    for i in (2, 0, 4, 3, 1):
        offs[i], at = at, at + nbs[i]
    rng = np.random.RandomState(12)
    pts = _plaintexts(rng, nbs, dls)
    cts = _encrypt_big(env, S, pts, 7202)
    d_in = B.to_device(cts, DEV)
    extra = 3  # rows past the sum(nb) output rows: not the call's to write
    ref = _oracle_extract(env, S, cts, nbs, dls, offs)
    for use_scratch in (False, True):
        d_out = torch.full((total + extra, p.n + 1), SENTINEL, dtype=torch.int64, device=DEV)
        scratch = None
        if use_scratch:
            need = B.extract_bits_scratch_bytes(p, len(nbs), max(nbs))
            scratch = torch.full(((need + 7) // 8,), SENTINEL, dtype=torch.int64, device=DEV)
        ret = B.extract_bits(p, S["fbsk"], S["ksk_dev"], d_in, nbs, dls, out=d_out, out_row_offsets=offs,
                             scratch=scratch)
        assert ret is d_out and B.stream_status(DEV) == 0
        got = B.to_host(d_out)
        assert np.array_equal(got[:total], ref), f"scratch={use_scratch}: output differs from the oracle"
        assert np.all(got[total:] == np.uint64(SENTINEL)), "rows outside the given blocks were written"
        assert np.array_equal(B.to_host(d_in), cts), "the input ciphertexts were modified"
    bits = _decrypt_bits(env, S, ref)
    for i, (pt, nb, dl) in enumerate(zip(pts, nbs, dls)):
        assert bits[int(offs[i]):int(offs[i]) + nb] == _expected_bits(pt, nb, dl), f"row {i}"
    # a scratch buffer one word short is refused, and nothing is written
    d_out = torch.full((total, p.n + 1), SENTINEL, dtype=torch.int64, device=DEV)
    short = torch.empty((B.extract_bits_scratch_bytes(p, len(nbs), max(nbs)) // 8 - 1,), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"\(-3\).*scratch"):
        B.extract_bits(p, S["fbsk"], S["ksk_dev"], d_in, nbs, dls, out=d_out, scratch=short)
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------
# 3. across the keyswitch's batch threshold (64 rows: matrix-core kernel above, VALU kernel below)
# ------------------------------------------------------------------------------------------------
def test_across_the_keyswitch_batch_threshold(env):
    B, torch = env["B"], env["torch"]
    S = _setup(env, "cfg2")
    rows = 70
    rng = np.random.RandomState(13)
    nbs = rng.randint(1, 4, size=rows).tolist()
    dls = [64 - nb for nb in nbs]
    active = [sum(nb > t for nb in nbs) for t in range(3)]
    assert active[0] >= 64 > active[1] > active[2] > 0, active  # the prefix crosses 64 rows between iterations
    pts = _plaintexts(rng, nbs, dls)
    d_in = B.to_device(_encrypt_big(env, S, pts, 7203), DEV)
    got = B.extract_bits(S["p"], S["fbsk"], S["ksk_dev"], d_in, nbs, dls)
    ref = _gpu_composition(env, S, d_in, nbs, dls)
    assert B.stream_status(DEV) == 0
    assert torch.equal(got, ref), f"{int((got != ref).sum())} words differ from the keyswitch / PBS composition"
    bits = _decrypt_bits(env, S, B.to_host(got))
    assert bits == [b for pt, nb, dl in zip(pts, nbs, dls) for b in _expected_bits(pt, nb, dl)]


# ------------------------------------------------------------------------------------------------
# 4. decrypt level, including cfg2's full n = 630
# ------------------------------------------------------------------------------------------------
# dl >= 58: the window margin 2^(dl-4) >= 2^54 stays far above the input noise (2^-25 of the torus: 2^39)
@pytest.mark.parametrize("name,rows,nb,dl", [("cfg2", 16, 5, 58), ("cfg4", 6, 3, 61), ("opt1", 6, 2, 62),
                                             ("cfg2_full", 8, 3, 61)])
def test_decrypted_bits(env, name, rows, nb, dl):
    B = env["B"]
    S = _setup(env, name)
    rng = np.random.RandomState(14)
    pts = _plaintexts(rng, [nb] * rows, [dl] * rows)
    d_in = B.to_device(_encrypt_big(env, S, pts, 7204), DEV)
    got = B.to_host(B.extract_bits(S["p"], S["fbsk"], S["ksk_dev"], d_in, nb, dl))
    assert B.stream_status(DEV) == 0
    bits = _decrypt_bits(env, S, got)
    assert bits == [b for pt in pts for b in _expected_bits(pt, nb, dl)]


# ------------------------------------------------------------------------------------------------
# 5. the CRT front end of the runtime's WoP-PBS
# ------------------------------------------------------------------------------------------------
def test_crt_front_end(env):
    B, torch = env["B"], env["torch"]
    S = _setup(env, "cfg2")
    p = S["p"]
    moduli = [3, 5, 7, 16]
    values = [0, 6, 11, 104, 1000, 3 * 5 * 7 * 16 - 1]
    nbs = [B.crt_bits(m) for m in moduli]
    assert nbs == [2, 3, 3, 4]
    pts = [B.crt_encode(v, m) for v in values for m in moduli]
    cts = _encrypt_big(env, S, pts, 7205).reshape(len(values), len(moduli), p.big_n + 1)
    d_blocks = B.to_device(cts, DEV)
    out = B.crt_extract_bits(p, S["fbsk"], S["ksk_dev"], d_blocks, moduli)
    assert B.stream_status(DEV) == 0
    assert tuple(out.shape) == (len(values), sum(nbs), p.n + 1)
    assert np.array_equal(B.to_host(d_blocks), cts), "the input blocks were modified"
    got = B.to_host(out)
    for j, v in enumerate(values):
        bits = _decrypt_bits(env, S, got[j])
        want = []
        for m, nb in reversed(list(zip(moduli, nbs))):  # [bits of block n-1 | ... | bits of block 0]
            r = ((v % m) << nb) // m
            want += [(r >> (nb - 1 - i)) & 1 for i in range(nb)]
        assert bits == want, f"v={v}"


# ------------------------------------------------------------------------------------------------
# 6. the reference-named trio on a cuda_create_stream stream
# ------------------------------------------------------------------------------------------------
def test_reference_named_trio(env):
    B, L = env["B"], env["L"]
    S = _setup(env, "cfg2")
    p = S["p"]
    rows, nb, dl = 6, 3, 61
    rng = np.random.RandomState(16)
    cts = _encrypt_big(env, S, _plaintexts(rng, [nb] * rows, [dl] * rows), 7206)
    out_words = rows * nb * (p.n + 1)
    bufs = dict(ksk=B.RuntimeBuffer(S["ksk"]), bsk=B.RuntimeBuffer(np.zeros(p.bsk_len, dtype=np.uint64)),
                inp=B.RuntimeBuffer(cts),
                **{k: B.RuntimeBuffer(np.zeros(out_words, dtype=np.uint64)) for k in ("trio", "pool", "ext")})
    stream = L.cuda_create_stream(0)
    try:
        bsk = np.ascontiguousarray(S["bsk"])
        L.cuda_convert_lwe_programmable_bootstrap_key_64(stream, 0, bufs["bsk"].ptr, bsk.ctypes.data, p.n, p.k, p.level,
                                                         p.N)
        fourier = L.concrete_hip_lookup_bsk(bufs["bsk"].ptr)
        assert fourier
        scratch = C.c_void_p()
        L.scratch_cuda_extract_bits_64(stream, 0, C.byref(scratch), p.k, p.n, p.N, p.level, rows, 0, True)
        assert scratch.value
        # the `dest` of the conversion as the key, scratch from the scratch call
        L.cuda_extract_bits_64(stream, 0, bufs["trio"].ptr, bufs["inp"].ptr, scratch, bufs["ksk"].ptr, bufs["bsk"].ptr,
                               nb, dl, p.big_n, p.n, p.k, p.N, p.base_log, p.level, p.ks_base_log, p.ks_level, rows, 0)
        L.cleanup_cuda_extract_bits(stream, 0, C.byref(scratch))
        assert not scratch.value
        # a caller-owned Fourier key and no buffer (pool scratch)
        L.cuda_extract_bits_64(stream, 0, bufs["pool"].ptr, bufs["inp"].ptr, None, bufs["ksk"].ptr, fourier, nb, dl,
                               p.big_n, p.n, p.k, p.N, p.base_log, p.level, p.ks_base_log, p.ks_level, rows, 0)
        nbs, dls = np.full(rows, nb, dtype=np.uint32), np.full(rows, dl, dtype=np.uint32)
        rc = L.concrete_hip_extract_bits(stream, 0, bufs["ext"].ptr, bufs["inp"].ptr, fourier, bufs["ksk"].ptr,
                                         nbs.ctypes.data, dls.ctypes.data, None, p.big_n, p.n, p.k, p.N, p.base_log,
                                         p.level, p.ks_base_log, p.ks_level, rows, None, 0)
        env["N"].check(rc, "concrete_hip_extract_bits")
        assert L.concrete_hip_stream_status(stream, 0) == 0
        host = {}
        for k in ("trio", "pool", "ext"):
            host[k] = np.zeros(out_words, dtype=np.uint64)
            L.cuda_memcpy_async_to_cpu(host[k].ctypes.data, bufs[k].ptr, host[k].nbytes, stream, 0)
        L.cuda_synchronize_device(0)
        assert host["ext"].any()
        assert np.array_equal(host["trio"], host["ext"]) and np.array_equal(host["pool"], host["ext"])
    finally:
        L.cuda_destroy_stream(stream, 0)
        for b in bufs.values():
            b.free()
