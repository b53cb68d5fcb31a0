"""The WoP-PBS end to end on the CPU: the definition the chained device calls are held to, word
for word.  A helper module, not a test file.  All arithmetic mod 2^64.

CRT front   block i of modulus m_i yields nb_i = ceil(log2 m_i) bits at delta_log 64 - nb_i, after
            2^(63-nb_i) - 2^(59-nb_i) is taken off its body (the second term dropped when nb_i > 59); per value
            the extracted rows are [bits of block n-1 | ... | bits of block 0], each most significant bit first
            (compiler lib/Runtime/wrappers.cpp:903-965).
extraction  the loop of tests/test_gpu_extract_bits.py's docstring on the oracle's integer keyswitch and
            Karatsuba PBS.
chain       t bit ciphertexts -> cbs_reference.circuit_bootstrap at delta_log 63 -> the GGSWs of
            vp_reference.vertical_packing at (level_cbs, base_log_cbs) with r = max(t - log2 N, 0) tree bits and
            m = min(t, log2 N) rotation bits, on the LUTs as [tau][2^r][N]: the [tau][2^t] array as it stands
            when t >= log2 N, else its 2^t words at the front of a zero polynomial.
"""
import os
import sys

import numpy as np

from oracle import pyoracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cbs_reference as R  # noqa: E402
import vp_reference as V  # noqa: E402

M64 = (1 << 64) - 1


def crt_bits(modulus):
    return (int(modulus) - 1).bit_length()


def crt_encode(v, modulus):
    """compiler lib/Common/CRT.cpp:80-88: floor((v mod m) 2^64 / m)."""
    return ((int(v) % int(modulus)) << 64) // int(modulus)


def crt_offset(nb):
    return ((1 << (63 - nb)) - ((1 << (59 - nb)) if nb <= 59 else 0)) & M64


def crt_front(blocks, moduli):
    """blocks (batch, nblk, kN+1) -> the private copy with every block's offset off its body."""
    out = np.ascontiguousarray(blocks, dtype=np.uint64).copy()
    for i, m in enumerate(moduli):
        out[:, i, -1] -= np.uint64(crt_offset(crt_bits(m)))
    return out


def rm(t, N):
    logn = int(N).bit_length() - 1
    return max(t - logn, 0), min(t, logn)


def lut_layout(luts, t, N):
    """(tau, 2^t) -> (tau, 2^r, N)."""
    luts = np.ascontiguousarray(luts, dtype=np.uint64)
    tau = luts.shape[0]
    assert luts.shape[1] == 1 << t
    r, _ = rm(t, N)
    if (1 << t) >= N:
        return luts.reshape(tau, 1 << r, N)
    out = np.zeros((tau, 1, N), dtype=np.uint64)
    out[:, 0, :1 << t] = luts
    return out


def _const_acc(k, N, e):
    acc = np.zeros((k + 1) * N, dtype=np.uint64)
    acc[k * N:] = np.uint64((-(1 << e)) & M64)
    return acc


def extract_bits(cts, bsk, ksk, nbs, dls, first, op):
    """cts (rows, kN+1); row i yields nbs[i] bits at dls[i] into output rows first[i] .. + nbs[i] - 1, most
    significant first.  op: the oracle's Params (n, k, N, BSK and KS decompositions)."""
    nbs, dls, first = np.asarray(nbs, np.int64), np.asarray(dls, np.int64), np.asarray(first, np.int64)
    out = np.zeros((int(nbs.sum()), op.n + 1), dtype=np.uint64)
    c = np.ascontiguousarray(cts, dtype=np.uint64).copy()
    for t in range(int(nbs.max())):
        act = np.nonzero(nbs > t)[0]
        sh = (64 - dls[act] - t - 1).astype(np.uint64)
        u = O.keyswitch_batch(op, c[act] << sh[:, None], ksk)
        out[first[act] + nbs[act] - 1 - t] = u
        go = nbs[act] > t + 1
        if not go.any():
            break
        rows, u = act[go], u[go].copy()
        u[:, -1] += np.uint64(1 << 62)
        exps = (dls[rows] - 1 + t).astype(np.int64)
        uniq = sorted(set(exps.tolist()))
        accs = np.stack([_const_acc(op.k, op.N, e) for e in uniq])
        lut_idx = np.array([uniq.index(e) for e in exps.tolist()], dtype=np.uint64)
        v, _ = O.pbs_batch(op, u, accs, bsk=bsk, lut_idx=lut_idx, mode=O.MODE_KARATSUBA)
        v[:, -1] += np.uint64(1) << exps.astype(np.uint64)
        c[rows] -= v
    return out


def crt_extract(blocks, moduli, bsk, ksk, op):
    """blocks (batch, nblk, kN+1) -> (batch, t, n+1), per value [bits of block n-1 | ... | bits of block 0]."""
    batch, nblk = blocks.shape[0], blocks.shape[1]
    nbs = [crt_bits(m) for m in moduli]
    t = sum(nbs)
    first = np.concatenate([np.cumsum(nbs[::-1])[::-1][1:], [0]]).astype(np.int64)
    offs = (np.arange(batch, dtype=np.int64)[:, None] * t + first[None, :]).reshape(-1)
    flat = crt_front(blocks, moduli).reshape(batch * nblk, -1)
    out = extract_bits(flat, bsk, ksk, np.tile(nbs, batch), np.tile([64 - nb for nb in nbs], batch), offs, op)
    return out.reshape(batch, t, op.n + 1)


def cbs_vp(bits, luts, bsk, fpksk, op, pksk, cbs):
    """bits (lookups, t, n+1) at 2^63; luts (tau, 2^t); pksk, cbs = (level, base_log) -> (lookups, tau, kN+1)."""
    lookups, t = bits.shape[0], bits.shape[1]
    k, N = op.k, op.N
    ggsw, _ = R.circuit_bootstrap(bits.reshape(lookups * t, op.n + 1), bsk, fpksk, 63, op.n, k, N, op.l, op.logB,
                                  pksk[0], pksk[1], cbs[0], cbs[1])
    r, m = rm(t, N)
    lwe, _ = V.vertical_packing(ggsw.reshape(lookups, t, cbs[0], k + 1, k + 1, N), lut_layout(luts, t, N), r, m, k, N,
                                cbs[0], cbs[1])
    return lwe


def wop_pbs_crt(blocks, luts, moduli, bsk, ksk, fpksk, op, pksk, cbs):
    """The whole chain: blocks (batch, nblk, kN+1), luts (nblk, 2^t) -> (batch, nblk, kN+1)."""
    return cbs_vp(crt_extract(blocks, moduli, bsk, ksk, op), luts, bsk, fpksk, op, pksk, cbs)


def selected_index(value, moduli):
    """The LUT index the extracted bits of `value` name: per block the top nb_i bits of its CRT encoding,
    floor((value mod m_i) 2^nb_i / m_i), block n-1 most significant."""
    idx = 0
    for m in reversed(list(moduli)):
        nb = crt_bits(m)
        idx = (idx << nb) | (crt_encode(value, m) >> (64 - nb))
    return idx
