"""Vertical packing (WoP-PBS stage 3) on the CPU: the definition the device code is held to,
word for word.  A helper module, not a test file.

With cmux(c0, c1, G) = c0 + G [x] (c1 - c0), [x] = oracle/tfhe_oracle.c:ora_external_product_acc in its integer
mode, and all arithmetic mod 2^64, one lookup is

  tree      leaves: the trivial GLWEs of the 2^r LUT polynomials of an output.  Layer j = 0 .. r-1 uses tree
            GGSW r-1-j (the list is most significant bit first); its node i is cmux(prev[2i], prev[2i+1], G).
  rotation  for j = m-1 down to 0, d = 2^(m-1-j): acc = cmux(acc, X^(-d) acc, G_j).
  extract   ora_sample_extract of the result.

The rotation runs on code the oracle already has: a PBS whose bootstrapping key is the rotation GGSWs in the
order they are applied (entry i = G_(m-1-i)) and whose input is one synthetic LWE row with
a_i = (2N - 2^i) << (64 - log2 2N) and b = 0.  The modulus switch reproduces 2N - 2^i exactly, X^(2N - d) =
X^(-d), and the PBS step acc += G [x] (X^a acc - acc) is the CMUX above.  `rotate_direct` is the same loop
written out with ora_monomial_div; tests/test_vertical_packing_abi.py holds the two against each other.
"""
import ctypes as C

import numpy as np

from oracle import pyoracle as O

u64p = C.POINTER(C.c_uint64)
sz = C.c_size_t


def limb_bits(k, N, level):
    """Limb width of the general key format of (k, N, level) (pbs_generic.hip:generic_limb_bits)."""
    from oracle import keyref
    return keyref.generic_limb_bits(k, N, level)


def error_bound(k, N, level, base_log, max_g=None):
    """The general path's certified rounding bound for GGSWs whose largest limb-spectrum magnitude is max_g
    (None: the random-key estimate of the static gate).  concrete_hip_generic_error_bound answers only for
    shapes whose primary key format is the general one; this is the same function (tests/test_oracle.py
    holds the two together) for every shape."""
    bits = limb_bits(k, N, level)
    spec = None if max_g is None else np.array([max_g / (N / 2.0), 0.0])
    return O.generic_error_bound(k, N, level, base_log, bits, spec)


def generic_pbs_ok(k, N, level, base_log):
    """pbs_generic.hip:generic_pbs_ok, restated on the oracle's bound."""
    if not (1 <= k <= 8 and 1 <= level <= 64 and 256 <= N <= 65536 and N & (N - 1) == 0):
        return False
    bits = limb_bits(k, N, level)
    if bits == 0 or -(-64 // bits) > 8 or base_log < 1 or level * base_log > 64:
        return False
    return error_bound(k, N, level, base_log) < 0.25


def ggsw_words(k, N, level):
    return level * (k + 1) * (k + 1) * N


def ggsw_encrypt(glwe_sk, bits, k, N, level, base_log, std, seed):
    """One GGSW per entry of the integer array `bits` (any shape): shape + (level, k+1, k+1, N) u64, level
    matrix 0 being decomposition level 1, as one entry of a standard bootstrapping key."""
    L = O.lib()
    L.ora_ggsw_encrypt.argtypes = [u64p, u64p, C.c_uint64, sz, sz, sz, sz, C.c_double, C.c_void_p]
    L.ora_ggsw_encrypt.restype = None
    bits = np.asarray(bits, dtype=np.int64)
    out = np.zeros((bits.size, ggsw_words(k, N, level)), dtype=np.uint64)
    sk = np.ascontiguousarray(glwe_sk, dtype=np.uint64)
    for i, b in enumerate(bits.reshape(-1)):
        r = (C.c_uint64 * 6)()
        L.ora_rng_seed(C.byref(r), C.c_uint64(seed + 977 * i))
        L.ora_ggsw_encrypt(O.P(sk), out[i].ctypes.data_as(u64p), C.c_uint64(int(b)), k, N, level, base_log, std,
                           C.byref(r))
    return out.reshape(bits.shape + (level, k + 1, k + 1, N))


def cmux(c0, c1, G, k, N, level, base_log):
    acc = np.ascontiguousarray(c0, dtype=np.uint64).copy()
    ct1 = np.ascontiguousarray(c1, dtype=np.uint64) - acc
    resid = C.c_double(0.0)
    O.lib().ora_external_product_acc(O.P(acc), O.P(np.ascontiguousarray(G, dtype=np.uint64).reshape(-1)), None,
                                     O.P(ct1), k, N, level, base_log, 3, O.MODE_KARATSUBA, C.byref(resid))
    return acc


def tree(ggsws, luts, k, N, level, base_log):
    """ggsws (r, level, k+1, k+1, N); luts (tau, 2^r, N) -> (tau, (k+1)N)."""
    r, tau = ggsws.shape[0], luts.shape[0]
    assert luts.shape[1] == 1 << r
    out = np.zeros((tau, (k + 1) * N), dtype=np.uint64)
    for o in range(tau):
        nodes = np.zeros((1 << r, (k + 1) * N), dtype=np.uint64)
        nodes[:, k * N:] = luts[o]
        for j in range(r):
            G = ggsws[r - 1 - j]
            nodes = np.stack([cmux(nodes[2 * i], nodes[2 * i + 1], G, k, N, level, base_log)
                              for i in range(nodes.shape[0] // 2)])
        out[o] = nodes[0]
    return out


def sample_extract(glwes, k, N):
    glwes = np.ascontiguousarray(glwes, dtype=np.uint64)
    out = np.zeros((glwes.shape[0], k * N + 1), dtype=np.uint64)
    for i in range(glwes.shape[0]):
        O.lib().ora_sample_extract(out[i].ctypes.data_as(u64p), glwes[i].ctypes.data_as(u64p), k, N)
    return out


def synthetic_lwe(m, N):
    """The LWE row that makes a PBS over m GGSWs rotate by X^(-2^i) at step i: a_i = 2N - 2^i, b = 0."""
    log2_2n = int(N).bit_length()  # log2(2N)
    row = np.zeros(m + 1, dtype=np.uint64)
    for i in range(m):
        row[i] = np.uint64(((2 * N - (1 << i)) << (64 - log2_2n)) & ((1 << 64) - 1))
    return row


def pbs_key(ggsws_rot):
    """The rotation GGSWs (m, level, k+1, k+1, N) as a standard bootstrapping key in application order."""
    return np.ascontiguousarray(ggsws_rot[::-1]).reshape(-1)


def rotate_extract(glwes, ggsws_rot, k, N, level, base_log):
    """glwes (tau, (k+1)N); ggsws_rot (m, ...) -> (tau, kN+1): the rotation as a PBS, then the extraction."""
    m = ggsws_rot.shape[0]
    if m == 0:
        return sample_extract(glwes, k, N)
    p = O.Params(n=m, k=k, N=N, l=level, logB=base_log)
    tau = glwes.shape[0]
    rows = np.tile(synthetic_lwe(m, N), (tau, 1))
    out, _ = O.pbs_batch(p, rows, glwes, bsk=pbs_key(ggsws_rot), lut_idx=np.arange(tau, dtype=np.uint64),
                         mode=O.MODE_KARATSUBA)
    return out


def rotate_direct(glwes, ggsws_rot, k, N, level, base_log):
    """The rotation loop of the definition, written out: (tau, (k+1)N) -> (tau, (k+1)N)."""
    L = O.lib()
    m = ggsws_rot.shape[0]
    out = np.ascontiguousarray(glwes, dtype=np.uint64).copy()
    for o in range(out.shape[0]):
        acc = out[o].copy()
        for j in range(m - 1, -1, -1):
            d = 1 << (m - 1 - j)
            rot = np.zeros_like(acc)
            for c in range(k + 1):
                L.ora_monomial_div(rot[c * N:(c + 1) * N].ctypes.data_as(u64p),
                                   acc[c * N:(c + 1) * N].ctypes.data_as(u64p), d, N)
            acc = cmux(acc, rot, ggsws_rot[j], k, N, level, base_log)
        out[o] = acc
    return out


def vertical_packing(ggsws, luts, r, m, k, N, level, base_log):
    """ggsws (lookups, r + m, level, k+1, k+1, N), the tree's first; luts (tau, 2^r, N).
    Returns (lwe (lookups, tau, kN+1), tree result (lookups, tau, (k+1)N))."""
    lookups, tau = ggsws.shape[0], luts.shape[0]
    assert ggsws.shape[1] == r + m
    lwe = np.zeros((lookups, tau, k * N + 1), dtype=np.uint64)
    glwe = np.zeros((lookups, tau, (k + 1) * N), dtype=np.uint64)
    for lk in range(lookups):
        glwe[lk] = tree(ggsws[lk, :r], luts, k, N, level, base_log)
        lwe[lk] = rotate_extract(glwe[lk], ggsws[lk, r:], k, N, level, base_log)
    return lwe, glwe


def selected(luts, bits_tree, bits_rot):
    """(polynomial index, coefficient index) the GGSW bits select: both most significant bit first."""
    pi = 0
    for b in bits_tree:
        pi = 2 * pi + int(b)
    ci = 0
    for b in bits_rot:
        ci = 2 * ci + int(b)
    return pi, ci
