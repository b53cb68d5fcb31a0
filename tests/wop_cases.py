"""The small WoP-PBS cases (shape A of DESIGN.md §4.22) shared by tests/test_wop_pbs_abi.py, which settles their
decryption margin on the CPU reference, and tests/test_gpu_wop_pbs.py, which holds the device to the same words.
A helper module, not a test file.  Keys, inputs and the reference are made once per process and are read-only.

Shape A: k = 1, N = 512, n = 8, BSK (2, 10), KS (4, 4), fp-ks (2, 15) with a real key, CBS (4, 5), key noise
2^-52, input noise 2^-25.  Three CRT decompositions: [3, 4, 5] (t = 7 < log2 N: the LUT is padded, no tree),
[8, 8, 8] (t = 9 = log2 N: neither padding nor tree), [5, 7, 8, 9] (t = 13: r = 4, m = 9).  Three values each,
0 among them: its blocks sit exactly at the lower edge of the extraction window.
"""
import functools
import os
import sys

import numpy as np

from concrete_amd import backend as B
from oracle import pyoracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wop_reference as W  # noqa: E402

K, N, LWE_N = 1, 512, 8
BSK, KS, PKSK, CBS = (2, 10), (4, 4), (2, 15), (4, 5)
KEY_STD, INPUT_STD = 2.0 ** -52, 2.0 ** -25
MODULI_SETS = ((3, 4, 5), (8, 8, 8), (5, 7, 8, 9))
BATCH = 3
WIDTH = 2  # message bits of a LUT entry, at the top of the word
P = B.PbsParams(n=LWE_N, k=K, N=N, level=BSK[0], base_log=BSK[1], ks_level=KS[0], ks_base_log=KS[1])
OP = O.Params(n=LWE_N, k=K, N=N, l=BSK[0], logB=BSK[1], ks_l=KS[0], ks_logB=KS[1])


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def keys():
    O.lib()
    lwe_sk, glwe_sk = B.binary_key(LWE_N, 9901), B.binary_key(K * N, 9902)
    return _frozen(dict(lwe_sk=lwe_sk, glwe_sk=glwe_sk,
                        bsk=B.bsk_generate(P, lwe_sk, glwe_sk, 9903, std=KEY_STD),
                        ksk=B.ksk_generate(P, glwe_sk, lwe_sk, 9904, std=KEY_STD),
                        fpksk=B.fpksk_generate(P, glwe_sk, PKSK[0], PKSK[1], 9905, std=KEY_STD)))


@functools.lru_cache(maxsize=None)
def case(moduli):
    """values (BATCH,), blocks (BATCH, nblk, kN+1), table / luts (nblk, 2^t), index (BATCH,): the LUT entry each value
    selects, want (BATCH, nblk, kN+1): the reference chain's output.  A smaller batch is a prefix."""
    k = keys()
    seed = 9910 + 10 * MODULI_SETS.index(moduli)
    rng = np.random.RandomState(seed)
    prod = int(np.prod(moduli))
    values = [0] + [int(v) for v in rng.randint(1, prod, size=BATCH - 1)]
    pts = np.array([W.crt_encode(v, m) for v in values for m in moduli], dtype=np.uint64)
    blocks = B.lwe_encrypt(k["glwe_sk"], pts, K * N, INPUT_STD, seed + 1).reshape(BATCH, len(moduli), K * N + 1)
    t = sum(W.crt_bits(m) for m in moduli)
    table = rng.randint(0, 1 << WIDTH, size=(len(moduli), 1 << t)).astype(np.uint64)
    luts = table << np.uint64(64 - WIDTH)
    want = W.wop_pbs_crt(blocks, luts, moduli, k["bsk"], k["ksk"], k["fpksk"], OP, PKSK, CBS)
    index = np.array([W.selected_index(v, moduli) for v in values], dtype=np.int64)
    return _frozen(dict(values=np.array(values), blocks=blocks, table=table, luts=luts, want=want, index=index, t=t))


def decrypt(rows):
    """(rows, kN+1) under the big key -> the phases."""
    return O.lwe_decrypt_batch(keys()["glwe_sk"], np.ascontiguousarray(rows, dtype=np.uint64), K * N)


def messages(phases):
    return [((int(d) + (1 << (63 - WIDTH))) >> (64 - WIDTH)) % (1 << WIDTH) for d in phases]
