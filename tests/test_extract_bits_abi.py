"""The bit-extraction entry points (WoP-PBS stage 1) without a device: the support and
scratch-size queries, the refusals concrete_hip_extract_bits makes before its first device call, and the new
declarations of include/concrete_hip.h as C99 (tests/c_client/extract_bits_client.c)."""
import os
import shutil
import subprocess
from dataclasses import replace

import pytest

from concrete_amd import _native
from concrete_amd import backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "concrete_amd")

SETS = [B.CFG2, B.CFG4, B.OPTIMIZER_SETS[1], B.OPTIMIZER_SETS[4], B.OPTIMIZER_SETS[9],
        replace(B.CFG2, base_log=40),               # no PBS kernel takes 3 digits of 40 bits
        replace(B.CFG2, N=1000),                    # not a ring the backend has
        replace(B.CFG2, ks_level=4, ks_base_log=16),  # keyswitch: level * base_log = 64
        replace(B.CFG4, ks_level=7, ks_base_log=9)]


def test_symbols_are_bound():
    for name in ("scratch_cuda_extract_bits_64", "cuda_extract_bits_64", "cleanup_cuda_extract_bits",
                 "concrete_hip_extract_bits", "concrete_hip_extract_bits_scratch_bytes",
                 "concrete_hip_extract_bits_supported"):
        assert name in _native.SIGNATURES and name in _native.declared_symbols()
        getattr(_native.lib(), name)
    assert _native.lib().concrete_hip_abi_version() == 5  # the capability is found through _supported


@pytest.mark.parametrize("p", SETS, ids=lambda p: f"k{p.k}N{p.N}l{p.level}b{p.base_log}ks{p.ks_level}x{p.ks_base_log}")
def test_supported_agrees_with_pbs_and_keyswitch(p):
    L = _native.lib()
    both = bool(L.concrete_hip_pbs_supported(p.k, p.N, p.level, p.base_log)) and \
        bool(L.concrete_hip_keyswitch_supported(p.ks_level, p.ks_base_log, p.big_n, p.n))
    assert B.extract_bits_supported(p) == both
    # the keyswitch input must be the PBS output
    assert L.concrete_hip_extract_bits_supported(p.big_n + 1, p.n, p.k, p.N, p.base_log, p.level, p.ks_base_log,
                                                 p.ks_level) == 0


def test_both_outcomes_are_covered():
    got = {B.extract_bits_supported(p) for p in SETS}
    assert got == {True, False}


@pytest.mark.parametrize("p", [B.CFG2, B.CFG4, B.OPTIMIZER_SETS[1]], ids=["cfg2", "cfg4", "opt1"])
def test_scratch_bytes_grow_with_the_batch(p):
    sizes = [B.extract_bits_scratch_bytes(p, b, 4) for b in (1, 2, 3, 5, 64, 65, 4096)]
    assert sizes[0] > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    # the four row buffers alone: running copy, keyswitch input, PBS output, PBS input
    assert sizes[-1] >= 4096 * 8 * (3 * (p.big_n + 1) + p.n + 1)
    by_bits = [B.extract_bits_scratch_bytes(p, 5, nb) for nb in (1, 2, 8, 63)]
    assert all(a <= b for a, b in zip(by_bits, by_bits[1:]))
    assert B.extract_bits_scratch_bytes(p, 0, 4) == 0 and B.extract_bits_scratch_bytes(p, 5, 64) == 0


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not installed")
def test_c99_client_and_refusals_without_a_device(tmp_path):
    """The client compiles warning-free as C99 against the header and links the library; it then runs with
    every device hidden, so a refusal that reached a device call would abort instead of returning its code."""
    exe = tmp_path / "extract_bits_client"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_client", "extract_bits_client.c"), "-L", LIBDIR, "-lconcrete_hip",
                    f"-Wl,-rpath,{LIBDIR}", "-o", str(exe)], check=True)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "extract_bits_client ok" in out.stdout, out.stdout + out.stderr


def test_refusals_through_python():
    """The same codes reach Python as exceptions carrying the library's message."""
    import numpy as np

    class Fake:  # a device tensor stand-in: the refused call never touches it
        device = "cpu"
        shape = (2, B.CFG2.big_n + 1)

        def data_ptr(self):
            return 64

    L = _native.lib()
    nb, dl = np.array([2, 0], dtype=np.uint32), np.array([62, 63], dtype=np.uint32)
    p = B.CFG2
    rc = L.concrete_hip_extract_bits(None, 0, 64, 64, 64, 64, nb.ctypes.data, dl.ctypes.data, None, p.big_n, p.n, p.k,
                                     p.N, p.base_log, p.level, p.ks_base_log, p.ks_level, 2, None, 0)
    assert rc == -3
    with pytest.raises(RuntimeError, match="number_of_bits=0"):
        _native.check(rc, "concrete_hip_extract_bits")
    assert B.crt_encode(6, 7) == (6 << 64) // 7 and B.crt_encode(9, 7) == B.crt_encode(2, 7)
    assert [B.crt_bits(m) for m in (2, 3, 5, 7, 16, 17)] == [1, 2, 3, 3, 4, 5]
