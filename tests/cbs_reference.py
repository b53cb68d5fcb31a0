"""Circuit bootstrap (WoP-PBS stage 2) on the CPU: the definition the device code is held to,
word for word.  A helper module, not a test file.  All arithmetic mod 2^64.

fp-ks key list   [k+1 keys][kN+1 blocks][l][(k+1)N]; block j < kN belongs to bit s_j of the flattened GLWE key,
                 block kN to s_kN := -1; storage index t of a block holds decomposition level l - t (the order of
                 ora_ksk_generate).  Entry (i, j, t) is a GLWE encryption of -s_j 2^(64 - base_log level) P_i, with
                 P_i = polynomial i of the GLWE key for i < k and P_k the constant polynomial -1.
fp-ks            of one LWE row x (kN+1 words, body last) with key i: - sum_j sum_level d_{j,level} key[i][j][level],
                 d the balanced decomposition of every word, the body included; no body term is added.  That is
                 ora_keyswitch with n_in = kN+1, n_out + 1 = (k+1)N on the row (x, 0).
circuit bootstrap  of one LWE row c at delta_log; for v = 0 .. level_cbs-1, level = v+1:
                 u = c 2^(63 - delta_log), u.body += 2^62; w = PBS(u, acc_v), acc_v the trivial GLWE of the constant
                 -(2^(63 - base_log_cbs level)) in every coefficient; w.body += 2^(63 - base_log_cbs level); row i of
                 level matrix v of the GGSW = fp-ks of w with key i.  Level matrix 0 is decomposition level 1.
"""
import ctypes as C

import numpy as np

from oracle import pyoracle as O

u64p = C.POINTER(C.c_uint64)
sz = C.c_size_t
BLOCK_SEED = 0x2545f491  # block b = i (kN+1) + j has the stream seed ^ (BLOCK_SEED (b + 1)), as keygen.cpp
MASK = (1 << 64) - 1


def fpksk_words(k, N, level):
    return (k + 1) * (k * N + 1) * level * (k + 1) * N


def fpksk_generate(glwe_sk, k, N, level, base_log, std, seed):
    """(k+1, kN+1, level, (k+1)N) u64; the input LWE key is the flattened GLWE key."""
    L = O.lib()
    L.ora_glwe_encrypt_assign.argtypes = [u64p, u64p, sz, sz, C.c_double, C.c_void_p]
    L.ora_glwe_encrypt_assign.restype = None
    sk = np.ascontiguousarray(glwe_sk, dtype=np.uint64)
    blocks = k * N + 1
    out = np.zeros((k + 1, blocks, level, (k + 1) * N), dtype=np.uint64)
    for b in range((k + 1) * blocks):
        i, j = divmod(b, blocks)
        r = (C.c_uint64 * 6)()
        L.ora_rng_seed(C.byref(r), C.c_uint64((seed ^ (BLOCK_SEED * (b + 1))) & MASK))
        minus_s = (-int(sk[j])) & MASK if j < k * N else 1
        for t in range(level):
            factor = (minus_s << (64 - base_log * (level - t))) & MASK
            ct = out[i, j, t]
            if i < k:
                ct[k * N:] = sk[i * N:(i + 1) * N] * np.uint64(factor)
            else:
                ct[k * N] = np.uint64((-factor) & MASK)
            L.ora_glwe_encrypt_assign(O.P(sk), ct.ctypes.data_as(u64p), k, N, std, C.byref(r))
    return out


def fp_keyswitch(rows, fpksk, k, N, level, base_log):
    """rows (R, kN+1); fpksk (keys, kN+1, level, (k+1)N) -> (R, keys, (k+1)N): every row through every key."""
    L = O.lib()
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    R, W, G = rows.shape[0], k * N + 1, (k + 1) * N
    assert rows.shape[1] == W and fpksk.shape[1:] == (W, level, G)
    padded = np.zeros((R, W + 1), dtype=np.uint64)  # (x, 0)
    padded[:, :W] = rows
    out = np.zeros((R, fpksk.shape[0], G), dtype=np.uint64)
    for i in range(fpksk.shape[0]):
        one = np.zeros((R, G), dtype=np.uint64)
        L.ora_keyswitch_batch(O.P(one), None, O.P(padded), None, O.P(np.ascontiguousarray(fpksk[i]).reshape(-1)),
                              level, base_log, W, G - 1, R, 0)
        out[:, i] = one
    return out


def pbs_rows(lwe_in, bsk, delta_log, n, k, N, level_bsk, base_log_bsk, level_cbs, base_log_cbs):
    """Steps 1 to 3: (samples, n+1) -> (samples, level_cbs, kN+1), the rows the fp-ks reads."""
    lwe_in = np.ascontiguousarray(lwe_in, dtype=np.uint64)
    samples = lwe_in.shape[0]
    u = lwe_in << np.uint64(63 - delta_log)
    u[:, n] += np.uint64(1 << 62)
    accs = np.zeros((level_cbs, (k + 1) * N), dtype=np.uint64)
    consts = [1 << (63 - base_log_cbs * (v + 1)) for v in range(level_cbs)]
    for v in range(level_cbs):
        accs[v, k * N:] = np.uint64((-consts[v]) & MASK)
    p = O.Params(n=n, k=k, N=N, l=level_bsk, logB=base_log_bsk)
    w, _ = O.pbs_batch(p, np.repeat(u, level_cbs, axis=0), accs, bsk=bsk,
                       lut_idx=np.tile(np.arange(level_cbs, dtype=np.uint64), samples), mode=O.MODE_KARATSUBA)
    w = w.reshape(samples, level_cbs, k * N + 1)
    for v in range(level_cbs):
        w[:, v, k * N] += np.uint64(consts[v])
    return w


def circuit_bootstrap(lwe_in, bsk, fpksk, delta_log, n, k, N, level_bsk, base_log_bsk, level_pksk, base_log_pksk,
                      level_cbs, base_log_cbs):
    """(samples, n+1) -> (GGSWs (samples, level_cbs, k+1, (k+1)N), the fp-ks input rows (samples, level_cbs, kN+1));
    bsk the standard bootstrapping key, fpksk (k+1, kN+1, level_pksk, (k+1)N)."""
    w = pbs_rows(lwe_in, bsk, delta_log, n, k, N, level_bsk, base_log_bsk, level_cbs, base_log_cbs)
    samples = w.shape[0]
    ggsw = fp_keyswitch(w.reshape(samples * level_cbs, k * N + 1), fpksk[:k + 1], k, N, level_pksk, base_log_pksk)
    return ggsw.reshape(samples, level_cbs, k + 1, (k + 1) * N), w
