"""Host-side mirror of the runtime's use of the backend ABI (Python plumbing for tests/bench).

The reference runtime drives the backend from C++ (compiler lib/Runtime/wrappers.cpp:164-363,
GPUDFG.cpp:1114-1250, context.h:86-145).  This module replays that call sequence over the C
ABI with device memory owned by PyTorch (plumbing only: every computation is a HIP kernel of
libconcrete_hip.so).  Names follow the reference domain: LWE/GLWE ciphertexts, bootstrapping
key (BSK), keyswitching key (KSK), lookup tables (LUT).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native

vp = C.c_void_p


@dataclass(frozen=True)
class PbsParams:
    """n = LWE dimension of the PBS input, k = GLWE dimension, N = polynomial size,
    level/base_log = PBS decomposition, ks_level/ks_base_log = KS decomposition."""
    n: int
    k: int
    N: int
    level: int
    base_log: int
    ks_level: int = 4
    ks_base_log: int = 3

    @property
    def big_n(self) -> int:
        return self.k * self.N

    @property
    def lwe_in_size(self) -> int:
        return self.n + 1

    @property
    def lwe_out_size(self) -> int:
        return self.k * self.N + 1

    @property
    def glwe_size(self) -> int:
        return (self.k + 1) * self.N

    @property
    def bsk_len(self) -> int:  # u64 words, concrete-cpu bootstrap.rs:417-429
        return self.n * self.level * (self.k + 1) ** 2 * self.N

    @property
    def ksk_len(self) -> int:  # u64 words, concrete-cpu keyswitch.rs:226-236
        return self.big_n * self.ks_level * (self.n + 1)

    def bsk_bytes_per_pbs(self) -> int:
        """Algorithmic HBM bytes of one PBS: BSK + LWE in + LWE out."""
        return 8 * (self.bsk_len + self.lwe_in_size + self.lwe_out_size)


# BASELINE.json configs[1]/[2] (cfg2) and configs[3] (cfg4)
CFG2 = PbsParams(n=630, k=1, N=1024, level=3, base_log=7, ks_level=4, ks_base_log=3)
CFG4 = PbsParams(n=742, k=1, N=2048, level=1, base_log=23, ks_level=5, ks_base_log=3)

# The concrete optimizer's 128-bit parameter rows at log norm2 = 0 (compilers/concrete-optimizer/
# v0-parameters/ref/v0_last_128: k, log2 N, n, br_l, br_b, ks_l, ks_b), keyed by message bits.
# All but 5 bits run on the general path (pbs_generic.hip).
OPTIMIZER_SETS = {
    1: PbsParams(n=592, k=5, N=256, level=1, base_log=15, ks_level=3, ks_base_log=3),
    2: PbsParams(n=700, k=5, N=256, level=1, base_log=15, ks_level=3, ks_base_log=4),
    3: PbsParams(n=722, k=3, N=512, level=1, base_log=18, ks_level=3, ks_base_log=4),
    4: PbsParams(n=801, k=2, N=1024, level=1, base_log=23, ks_level=3, ks_base_log=4),
    5: PbsParams(n=783, k=1, N=2048, level=1, base_log=23, ks_level=5, ks_base_log=3),
    6: PbsParams(n=880, k=1, N=4096, level=1, base_log=22, ks_level=4, ks_base_log=4),
    7: PbsParams(n=915, k=1, N=8192, level=1, base_log=22, ks_level=6, ks_base_log=3),
    8: PbsParams(n=1006, k=1, N=16384, level=2, base_log=15, ks_level=5, ks_base_log=4),
    9: PbsParams(n=1039, k=1, N=32768, level=2, base_log=15, ks_level=7, ks_base_log=3),
    10: PbsParams(n=1136, k=1, N=65536, level=2, base_log=14, ks_level=6, ks_base_log=4),
}


def _ptr(a) -> int:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()  # torch tensor


# ---------------------------------------------------------------------------------------
# client-side generation (product keygen; deterministic per seed)
# ---------------------------------------------------------------------------------------
def secure_std(glwe_dim: int, poly_size: int) -> float:
    return 2.0 ** _native.lib().concrete_hip_secure_log2_std(glwe_dim, poly_size)


def binary_key(length: int, seed: int) -> np.ndarray:
    sk = np.zeros(length, dtype=np.uint64)
    _native.lib().concrete_hip_keygen_binary(_ptr(sk), length, seed)
    return sk


def lwe_encrypt(sk: np.ndarray, plaintexts, n: int, std: float, seed: int) -> np.ndarray:
    pts = np.ascontiguousarray(plaintexts, dtype=np.uint64)
    out = np.zeros((len(pts), n + 1), dtype=np.uint64)
    _native.lib().concrete_hip_lwe_encrypt_batch(_ptr(sk), _ptr(out), _ptr(pts), len(pts), n, std, seed)
    return out


def lwe_decrypt(sk: np.ndarray, cts: np.ndarray, n: int) -> np.ndarray:
    L = _native.lib()
    cts = np.ascontiguousarray(cts, dtype=np.uint64)
    return np.array([L.concrete_hip_lwe_decrypt(_ptr(sk), cts[i].ctypes.data, n) for i in range(cts.shape[0])],
                    dtype=np.uint64)


def bsk_generate(p: PbsParams, lwe_sk, glwe_sk, seed: int, std: float | None = None) -> np.ndarray:
    bsk = np.zeros(p.bsk_len, dtype=np.uint64)
    _native.lib().concrete_hip_bsk_generate(_ptr(bsk), _ptr(lwe_sk), _ptr(glwe_sk), p.n, p.k, p.N, p.level,
                                           p.base_log, secure_std(p.k, p.N) if std is None else std, seed)
    return bsk


def ksk_generate(p: PbsParams, sk_in, sk_out, seed: int, std: float | None = None) -> np.ndarray:
    ksk = np.zeros(p.ksk_len, dtype=np.uint64)
    _native.lib().concrete_hip_ksk_generate(_ptr(ksk), _ptr(sk_in), _ptr(sk_out), p.big_n, p.n, p.ks_level,
                                           p.ks_base_log, secure_std(1, p.n) if std is None else std, seed)
    return ksk


def encode(m, width: int):
    """Native integer encoding, compiler lib/Common/Transformers.cpp:364-382."""
    return np.uint64((int(m) << (64 - (width + 1))) & 0xFFFFFFFFFFFFFFFF)


def decode(x, width: int, signed: bool = False) -> int:
    """Native decoding, compiler lib/Common/Transformers.cpp:384-427 (signed: sign-extended)."""
    x = int(x)
    out = x >> (64 - width - 2)
    carry = out % 2
    out = ((out >> 1) + carry) % (1 << (width + 1))
    if signed and out >= (1 << (width - 1)):
        # Transformers.cpp:414-419: output |= UINT64_MAX << precision, read as int64
        out = (out & ((1 << width) - 1)) - (1 << width)
    return out


def expand_lut(table, N: int, out_bits: int, signed: bool = False) -> np.ndarray:
    tab = np.ascontiguousarray(table, dtype=np.uint64)
    out = np.zeros(N, dtype=np.uint64)
    _native.lib().concrete_hip_encode_expand_lut(_ptr(out), N, _ptr(tab), len(tab), out_bits, int(signed))
    return out


def trivial_glwe(p: PbsParams, lut_poly: np.ndarray) -> np.ndarray:
    """Trivial GLWE accumulator [0 .. 0 | LUT] (compiler lib/Runtime/wrappers.cpp:199-209)."""
    g = np.zeros(p.glwe_size, dtype=np.uint64)
    g[p.k * p.N:] = lut_poly
    return g


# ---------------------------------------------------------------------------------------
# device side (torch owns memory; kernels run on torch's current stream of that device)
# ---------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def to_device(a: np.ndarray, device):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(device)


def to_host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _stream(device) -> int:
    torch = _torch()
    return torch.cuda.current_stream(device).cuda_stream


def _gpu_index(device) -> int:
    torch = _torch()
    return torch.device(device).index or 0


class RuntimeBuffer:
    """A device buffer allocated and filled the way the reference runtime does it
    (cuda_malloc_async + cuda_memcpy_async_to_gpu, include/concretelang/Runtime/context.h:134-139),
    released by cuda_drop: the backend sees its lifetime, so derived data (the matrix-core
    keyswitch's key bytes) may be cached for it.  Has data_ptr() like a torch tensor."""

    def __init__(self, host: np.ndarray, gpu: int = 0):
        L = _native.lib()
        host = np.ascontiguousarray(host)
        self.gpu = gpu
        self.stream = L.cuda_create_stream(gpu)
        self.nbytes = host.nbytes
        self.ptr = L.cuda_malloc_async(self.nbytes, self.stream, gpu)
        self.write(host)

    def write(self, host: np.ndarray):
        L = _native.lib()
        host = np.ascontiguousarray(host)
        assert host.nbytes == self.nbytes
        L.cuda_memcpy_async_to_gpu(self.ptr, host.ctypes.data, self.nbytes, self.stream, self.gpu)
        L.cuda_synchronize_device(self.gpu)

    def data_ptr(self) -> int:
        return self.ptr

    def free(self):
        if self.ptr:
            L = _native.lib()
            L.cuda_drop(self.ptr, self.gpu)
            L.cuda_destroy_stream(self.stream, self.gpu)
            self.ptr = None


def pbs_supported(p: PbsParams) -> bool:
    """Whether the kernels take this parameter set (and compute it exactly: pbs.hpp)."""
    return bool(_native.lib().concrete_hip_pbs_supported(p.k, p.N, p.level, p.base_log))


def bsk_format(p: PbsParams) -> tuple[int, int, int]:
    """Device key format of (k, N, l): (kind, limbs, limb bits); kind 1 / 2 = the N = 1024 /
    2048 kernels' layouts, 3 = the general path (pbs_generic.hip), 0 = unsupported."""
    limbs, bits = C.c_uint32(0), C.c_uint32(0)
    kind = _native.lib().concrete_hip_bsk_format(p.k, p.N, p.level, C.byref(limbs), C.byref(bits))
    return int(kind), int(limbs.value), int(bits.value)


def fourier_bsk_bytes(p: PbsParams) -> int:
    return int(_native.lib().concrete_hip_fourier_bsk_size_bytes(p.n, p.k, p.level, p.N))


def convert_bsk(p: PbsParams, bsk, device="cuda:0", out=None):
    """Standard u64 BSK (numpy host array or torch device tensor) -> device Fourier key."""
    torch = _torch()
    nbytes = fourier_bsk_bytes(p)
    if out is None:
        out = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
    src_is_dev = not isinstance(bsk, np.ndarray)
    src = bsk if src_is_dev else np.ascontiguousarray(bsk, dtype=np.uint64)
    _native.check(_native.lib().concrete_hip_convert_bsk(_stream(device), _gpu_index(device), _ptr(out), _ptr(src),
                                                          int(src_is_dev), p.n, p.k, p.level, p.N),
                  "concrete_hip_convert_bsk")
    return out


def pbs(p: PbsParams, fbsk, lwe_in, luts, lut_idx=None, in_idx=None, out_idx=None, out=None,
        num_samples=None, resid=None):
    """Batched PBS on device tensors: lwe_in (B, n+1), luts (L, (k+1)N) -> out (B, kN+1)."""
    torch = _torch()
    device = lwe_in.device
    B = lwe_in.shape[0] if num_samples is None else num_samples
    if out is None:
        out = torch.empty((B, p.lwe_out_size), dtype=torch.int64, device=device)
    _native.check(_native.lib().concrete_hip_pbs(
        _stream(device), _gpu_index(device), _ptr(out), _ptr(out_idx), _ptr(luts), _ptr(lut_idx), _ptr(lwe_in),
        _ptr(in_idx), _ptr(fbsk), p.n, p.k, p.N, p.base_log, p.level, B, _ptr(resid)), "concrete_hip_pbs")
    return out


def device_status(device="cuda:0") -> int:
    """Synchronise the device and return (and clear) its sticky status: 0, or -4 when a PBS
    kernel's wave synchronisation gave up since the last check (concrete_hip_device_status)."""
    return int(_native.lib().concrete_hip_device_status(_gpu_index(device)))


def stream_status(device="cuda:0", stream=None) -> int:
    """Wait for the work issued on `stream` (default: torch's current stream of `device`) and return
    (and clear) the status of the PBS launches made on it: 0, or -4 when one gave up a wave
    synchronisation (concrete_hip_stream_status; status words are per stream)."""
    s = _stream(device) if stream is None else stream.cuda_stream
    return int(_native.lib().concrete_hip_stream_status(s, _gpu_index(device)))


def set_spin_limit(polls: int) -> None:
    """Spin bound of the PBS kernels' wave synchronisation (0 = default); a test hook."""
    _native.lib().concrete_hip_set_spin_limit(int(polls))


def set_thread_spin_limit(polls: int) -> None:
    """The same bound for launches issued by the calling thread only (0 = the process bound)."""
    _native.lib().concrete_hip_set_thread_spin_limit(int(polls))


def keyswitch(p: PbsParams, ksk_dev, lwe_in, out=None, in_idx=None, out_idx=None, num_samples=None):
    """Batched LWE keyswitch kN -> n on device tensors."""
    torch = _torch()
    device = lwe_in.device
    B = lwe_in.shape[0] if num_samples is None else num_samples
    if out is None:
        out = torch.empty((B, p.n + 1), dtype=torch.int64, device=device)
    _native.check(_native.lib().concrete_hip_keyswitch(
        _stream(device), _gpu_index(device), _ptr(out), _ptr(out_idx), _ptr(lwe_in), _ptr(in_idx), _ptr(ksk_dev),
        p.big_n, p.n, p.ks_base_log, p.ks_level, B), "concrete_hip_keyswitch")
    return out


# ---------------------------------------------------------------------------------------
# WoP-PBS stage 1: bit extraction (concrete_hip_extract_bits)
# ---------------------------------------------------------------------------------------
def extract_bits_supported(p: PbsParams) -> bool:
    return bool(_native.lib().concrete_hip_extract_bits_supported(p.big_n, p.n, p.k, p.N, p.base_log, p.level,
                                                                 p.ks_base_log, p.ks_level))


def extract_bits_scratch_bytes(p: PbsParams, num_samples: int, max_number_of_bits: int) -> int:
    return int(_native.lib().concrete_hip_extract_bits_scratch_bytes(p.big_n, p.n, p.k, p.N, num_samples,
                                                                     max_number_of_bits))


def _per_row(x, rows: int, what: str) -> np.ndarray:
    a = np.full(rows, x, dtype=np.uint32) if np.isscalar(x) else np.ascontiguousarray(x, dtype=np.uint32)
    if a.shape != (rows,):
        raise ValueError(f"{what}: {a.shape[0] if a.ndim == 1 else a.shape} entries for {rows} rows")
    return a


def extract_bits(p: PbsParams, fbsk, ksk_dev, lwe_in, number_of_bits, delta_log, out=None, out_row_offsets=None,
                 scratch=None):
    """Bit extraction on device tensors: lwe_in (B, kN+1) -> (sum nb, n+1) int64, per row the nb bits
    starting at bit dl, most significant first, each encrypted times 2^63 under the small key.
    number_of_bits / delta_log: ints or per-row sequences.  out_row_offsets: first output row of each
    input row's block (default: packed in input order).  lwe_in is not modified."""
    torch = _torch()
    device = lwe_in.device
    rows = lwe_in.shape[0]
    nb = _per_row(number_of_bits, rows, "number_of_bits")
    dl = _per_row(delta_log, rows, "delta_log")
    offs = None if out_row_offsets is None else np.ascontiguousarray(out_row_offsets, dtype=np.uint64)
    if offs is not None and offs.shape != (rows,):
        raise ValueError(f"out_row_offsets: {offs.shape} for {rows} rows")
    total = int(nb.astype(np.int64).sum())
    if out is None:
        out = torch.empty((total, p.n + 1), dtype=torch.int64, device=device)
    elif out.shape[0] < total or out.shape[1] != p.n + 1 or not out.is_contiguous():
        raise ValueError(f"out: need a contiguous (>= {total}, {p.n + 1}) tensor, got {tuple(out.shape)}")
    _native.check(_native.lib().concrete_hip_extract_bits(
        _stream(device), _gpu_index(device), _ptr(out), _ptr(lwe_in), _ptr(fbsk), _ptr(ksk_dev), _ptr(nb), _ptr(dl),
        _ptr(offs), p.big_n, p.n, p.k, p.N, p.base_log, p.level, p.ks_base_log, p.ks_level, rows,
        _ptr(scratch), 0 if scratch is None else scratch.numel() * scratch.element_size()),
        "concrete_hip_extract_bits")
    return out


def crt_encode(v: int, modulus: int) -> int:
    """CRT block encoding, compiler lib/Common/CRT.cpp:80-88: floor((v mod m) 2^64 / m)."""
    return ((int(v) % int(modulus)) << 64) // int(modulus)


def crt_bits(modulus: int) -> int:
    """Bits extracted from a block of this modulus: ceil(log2 m) (wrappers.cpp:908-909)."""
    return (int(modulus) - 1).bit_length()


def crt_extract_bits(p: PbsParams, fbsk, ksk_dev, blocks, moduli):
    """The bit-extraction front end of the runtime's CRT WoP-PBS (compiler lib/Runtime/wrappers.cpp:903-965)
    for a batch: blocks (batch, len(moduli), kN+1) -> (batch, sum nb_i, n+1), per value the reference's order
    [bits of block n-1 | ... | bits of block 0], each most significant bit first.  Block i yields
    nb_i = ceil(log2 m_i) bits at delta_log 64 - nb_i, after 2^(63-nb_i) - 2^(59-nb_i) is taken off its body."""
    torch = _torch()
    device = blocks.device
    batch, nblk = blocks.shape[0], blocks.shape[1]
    assert nblk == len(moduli) and blocks.shape[2] == p.big_n + 1
    nbs = [crt_bits(m) for m in moduli]
    assert min(nbs) >= 1, "a CRT modulus must be at least 2"
    per_value = sum(nbs)
    flat = blocks.reshape(batch * nblk, p.big_n + 1)
    sub = np.array([(-((1 << (63 - nb)) - ((1 << (59 - nb)) if nb <= 59 else 0))) % (1 << 64) for nb in nbs],
                   dtype=np.uint64)
    shifted = torch.empty_like(flat)
    _native.lib().cuda_add_lwe_ciphertext_vector_plaintext_vector_64(
        _stream(device), _gpu_index(device), _ptr(shifted), _ptr(flat), _ptr(to_device(np.tile(sub, batch), device)),
        p.big_n, batch * nblk)
    # block i of a value lands after the blocks above it
    first = np.concatenate([np.cumsum(nbs[::-1])[::-1][1:], [0]]).astype(np.uint64)
    offs = (np.arange(batch, dtype=np.uint64)[:, None] * np.uint64(per_value) + first[None, :]).reshape(-1)
    out = extract_bits(p, fbsk, ksk_dev, shifted, np.tile(nbs, batch), np.tile([64 - nb for nb in nbs], batch),
                       out_row_offsets=offs)
    return out.reshape(batch, per_value, p.n + 1)


# ---------------------------------------------------------------------------------------
# WoP-PBS stage 3: vertical packing (concrete_hip_vertical_packing)
# ---------------------------------------------------------------------------------------
def vertical_packing_supported(p: PbsParams) -> bool:
    return bool(_native.lib().concrete_hip_vertical_packing_supported(p.k, p.N, p.level, p.base_log))


def vertical_packing_scratch_bytes(p: PbsParams, r: int, mbr_size: int, tau: int, num_lookups: int = 1) -> int:
    return int(_native.lib().concrete_hip_vertical_packing_scratch_bytes(p.k, p.N, p.level, r, mbr_size, tau,
                                                                         num_lookups))


def vertical_packing(p: PbsParams, ggsw, luts, r: int, mbr_size: int, num_lookups: int = 1, out=None, tree_out=None,
                     scratch=None, resid=None, want_tree: bool = False):
    """Vertical packing on device tensors.  ggsw: (num_lookups, r + mbr_size, level, k+1, k+1, N) standard
    GGSWs, the tree's first, most significant bit first (None when r + mbr_size == 0); luts: (tau, 2^r, N),
    shared by the lookups.  Returns (lwe, tree, max|G|): lwe (num_lookups, tau, kN+1) int64; tree
    (num_lookups, tau, (k+1)N), the CMUX tree's result, when tree_out is given or want_tree is set, else None;
    max|G| the measured spectrum magnitude of the converted GGSWs.  p.n is not used."""
    torch = _torch()
    device = luts.device
    tau = luts.shape[0]
    if luts.shape[1] != 1 << r or luts.shape[2] != p.N or not luts.is_contiguous():
        raise ValueError(f"luts: need a contiguous ({tau}, {1 << r}, {p.N}) tensor, got {tuple(luts.shape)}")
    words = num_lookups * (r + mbr_size) * p.level * (p.k + 1) ** 2 * p.N
    if words and (ggsw is None or ggsw.numel() != words or not ggsw.is_contiguous()):
        raise ValueError(f"ggsw: need {words} contiguous words for {num_lookups} x {r + mbr_size} GGSWs")
    if out is None:
        out = torch.empty((num_lookups, tau, p.lwe_out_size), dtype=torch.int64, device=device)
    if tree_out is None and want_tree:
        tree_out = torch.empty((num_lookups, tau, p.glwe_size), dtype=torch.int64, device=device)
    max_g = C.c_double(0.0)
    _native.check(_native.lib().concrete_hip_vertical_packing(
        _stream(device), _gpu_index(device), _ptr(out), _ptr(tree_out), _ptr(ggsw) if words else None, _ptr(luts),
        p.k, p.N, p.base_log, p.level, r, mbr_size, tau, num_lookups, _ptr(scratch),
        0 if scratch is None else scratch.numel() * scratch.element_size(), _ptr(resid), C.byref(max_g)),
        "concrete_hip_vertical_packing")
    return out, tree_out, max_g.value


# ---------------------------------------------------------------------------------------
# WoP-PBS stage 2: circuit bootstrap and its fp-ks (concrete_hip_circuit_bootstrap)
# ---------------------------------------------------------------------------------------
def fpksk_words(k: int, N: int, level: int) -> int:
    return int(_native.lib().concrete_hip_fpksk_size_words(k, N, level))


def fpksk_generate(p: PbsParams, glwe_sk, level: int, base_log: int, seed: int, std: float | None = None) -> np.ndarray:
    """The list of k + 1 fp-ks keys, (k+1, kN+1, level, (k+1)N) u64, from the flattened GLWE key (the PBS
    output's LWE key) to the same GLWE key."""
    sk = np.ascontiguousarray(glwe_sk, dtype=np.uint64)
    out = np.zeros((p.k + 1, p.big_n + 1, level, p.glwe_size), dtype=np.uint64)
    assert out.size == fpksk_words(p.k, p.N, level)
    _native.lib().concrete_hip_fpksk_generate(_ptr(out), _ptr(sk), _ptr(sk), p.k, p.N, level, base_log,
                                             secure_std(p.k, p.N) if std is None else std, seed)
    return out


def fp_keyswitch(k: int, N: int, level: int, base_log: int, fpksk_dev, lwe_in, num_keys: int | None = None, out=None):
    """fp-ks on device tensors: every row of lwe_in (rows, kN+1) through each of num_keys (default k + 1) keys of
    fpksk_dev -> (rows, num_keys, (k+1)N) int64."""
    torch = _torch()
    device = lwe_in.device
    rows = lwe_in.shape[0]
    nk = k + 1 if num_keys is None else num_keys
    if lwe_in.shape[1] != k * N + 1 or not lwe_in.is_contiguous():
        raise ValueError(f"lwe_in: need a contiguous (rows, {k * N + 1}) tensor, got {tuple(lwe_in.shape)}")
    if out is None:
        out = torch.empty((rows, nk, (k + 1) * N), dtype=torch.int64, device=device)
    _native.check(_native.lib().concrete_hip_fp_keyswitch(
        _stream(device), _gpu_index(device), _ptr(out), _ptr(lwe_in), _ptr(fpksk_dev), k * N, k, N, base_log, level,
        rows, nk), "concrete_hip_fp_keyswitch")
    return out


def circuit_bootstrap_supported(p: PbsParams, pksk_level: int, pksk_base_log: int, cbs_level: int,
                                cbs_base_log: int) -> bool:
    return bool(_native.lib().concrete_hip_circuit_bootstrap_supported(p.k, p.N, p.level, p.base_log, pksk_level,
                                                                      pksk_base_log, cbs_level, cbs_base_log))


def circuit_bootstrap_scratch_bytes(p: PbsParams, cbs_level: int, num_samples: int) -> int:
    return int(_native.lib().concrete_hip_circuit_bootstrap_scratch_bytes(p.n, p.k, p.N, cbs_level, num_samples))


def circuit_bootstrap(p: PbsParams, fbsk, fpksk_dev, lwe_in, delta_log: int, pksk_level: int, pksk_base_log: int,
                      cbs_level: int, cbs_base_log: int, out=None, scratch=None, pbs_out=None):
    """Circuit bootstrap on device tensors: lwe_in (samples, n+1), the bit at delta_log -> GGSWs
    (samples, cbs_level, k+1, (k+1)N) int64, level matrix 0 being decomposition level 1 (what vertical_packing
    reads).  pbs_out: optional (samples, cbs_level, kN+1) tensor that receives the rows the fp-ks reads."""
    torch = _torch()
    device = lwe_in.device
    samples = lwe_in.shape[0]
    if lwe_in.shape[1] != p.n + 1 or not lwe_in.is_contiguous():
        raise ValueError(f"lwe_in: need a contiguous (samples, {p.n + 1}) tensor, got {tuple(lwe_in.shape)}")
    if out is None:
        out = torch.empty((samples, cbs_level, p.k + 1, p.glwe_size), dtype=torch.int64, device=device)
    _native.check(_native.lib().concrete_hip_circuit_bootstrap(
        _stream(device), _gpu_index(device), _ptr(out), _ptr(lwe_in), _ptr(fbsk), _ptr(fpksk_dev), delta_log, p.n, p.k,
        p.N, p.level, p.base_log, pksk_level, pksk_base_log, cbs_level, cbs_base_log, samples, _ptr(scratch),
        0 if scratch is None else scratch.numel() * scratch.element_size(), _ptr(pbs_out)),
        "concrete_hip_circuit_bootstrap")
    return out


# ---------------------------------------------------------------------------------------
# The WoP-PBS end to end: chained drivers (concrete_hip_wop_pbs_crt)
# ---------------------------------------------------------------------------------------
def wop_pbs_supported(p: PbsParams, pksk_level: int, pksk_base_log: int, cbs_level: int, cbs_base_log: int) -> bool:
    """The conjunction of the three stages' _supported predicates for what the chain hands them."""
    return bool(_native.lib().concrete_hip_wop_pbs_supported(p.n, p.k, p.N, p.level, p.base_log, p.ks_level,
                                                            p.ks_base_log, pksk_level, pksk_base_log, cbs_level,
                                                            cbs_base_log))


def wop_pbs_scratch_bytes(p: PbsParams, cbs_level: int, num_blocks: int, number_of_bits: int, tau: int,
                          batch: int = 1) -> int:
    """Scratch bytes of a chained call: `batch` values of number_of_bits boolean inputs and tau LUTs, num_blocks
    stage-1 inputs per value (0: circuit_bootstrap_vertical_packing, which has no stage 1)."""
    return int(_native.lib().concrete_hip_wop_pbs_scratch_bytes(p.n, p.k, p.N, cbs_level, num_blocks, number_of_bits,
                                                                tau, batch))


def _scratch_args(scratch):
    return _ptr(scratch), 0 if scratch is None else scratch.numel() * scratch.element_size()


def circuit_bootstrap_vertical_packing(p: PbsParams, fbsk, fpksk_dev, bits, luts, pksk_level: int, pksk_base_log: int,
                                       cbs_level: int, cbs_base_log: int, out=None, scratch=None):
    """Stages 2 and 3 on device tensors: bits (lookups, t, n+1), the bit ciphertexts at 2^63, most significant
    first; luts (tau, 2^t) cleartext words shared by the lookups -> ((lookups, tau, kN+1) int64, max|G|)."""
    torch = _torch()
    device = bits.device
    lookups, t = bits.shape[0], bits.shape[1]
    tau = luts.shape[0]
    if bits.shape[2] != p.n + 1 or not bits.is_contiguous():
        raise ValueError(f"bits: need a contiguous (lookups, t, {p.n + 1}) tensor, got {tuple(bits.shape)}")
    if luts.shape[1] != 1 << t or not luts.is_contiguous():
        raise ValueError(f"luts: need a contiguous ({tau}, {1 << t}) tensor, got {tuple(luts.shape)}")
    if out is None:
        out = torch.empty((lookups, tau, p.lwe_out_size), dtype=torch.int64, device=device)
    max_g = C.c_double(0.0)
    _native.check(_native.lib().concrete_hip_circuit_bootstrap_vertical_packing(
        _stream(device), _gpu_index(device), _ptr(out), _ptr(bits), _ptr(luts), _ptr(fbsk), _ptr(fpksk_dev), p.n, p.k,
        p.N, p.level, p.base_log, pksk_level, pksk_base_log, cbs_level, cbs_base_log, t, tau, lookups,
        *_scratch_args(scratch), C.byref(max_g)), "concrete_hip_circuit_bootstrap_vertical_packing")
    return out, max_g.value


def wop_pbs_crt(p: PbsParams, fbsk, ksk_dev, fpksk_dev, blocks, luts, moduli, pksk_level: int, pksk_base_log: int,
                cbs_level: int, cbs_base_log: int, out=None, scratch=None):
    """The CRT WoP-PBS on device tensors: blocks (batch, len(moduli), kN+1), luts (len(moduli), 2^t) cleartext
    words with t = sum crt_bits(m_i) -> ((batch, len(moduli), kN+1) int64, max|G|).  blocks is not modified."""
    torch = _torch()
    device = blocks.device
    batch, nblk = blocks.shape[0], blocks.shape[1]
    mods = np.ascontiguousarray(moduli, dtype=np.uint64)
    t = sum(crt_bits(m) for m in moduli)
    if nblk != len(mods) or blocks.shape[2] != p.big_n + 1 or not blocks.is_contiguous():
        raise ValueError(f"blocks: need a contiguous (batch, {len(mods)}, {p.big_n + 1}) tensor, got {tuple(blocks.shape)}")
    if tuple(luts.shape) != (nblk, 1 << t) or not luts.is_contiguous():
        raise ValueError(f"luts: need a contiguous ({nblk}, {1 << t}) tensor, got {tuple(luts.shape)}")
    if out is None:
        out = torch.empty((batch, nblk, p.lwe_out_size), dtype=torch.int64, device=device)
    max_g = C.c_double(0.0)
    _native.check(_native.lib().concrete_hip_wop_pbs_crt(
        _stream(device), _gpu_index(device), _ptr(out), _ptr(blocks), _ptr(luts), _ptr(fbsk), _ptr(ksk_dev),
        _ptr(fpksk_dev), _ptr(mods), nblk, batch, p.n, p.k, p.N, p.level, p.base_log, p.ks_level, p.ks_base_log,
        pksk_level, pksk_base_log, cbs_level, cbs_base_log, *_scratch_args(scratch), C.byref(max_g)),
        "concrete_hip_wop_pbs_crt")
    return out, max_g.value
