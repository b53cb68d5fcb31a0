"""GPU tests on worst-case keys and digits (tests/worst_case.py): every PBS kernel instantiation
and every keyswitch product path, word for word against the oracle's integer arithmetic (oracle.pbs_batch in
Karatsuba mode, oracle.keyswitch_batch).  There is no tolerance anywhere.

Each PBS case runs three legs on the worst-case batch of nine ciphertexts (three at N >= 32768):
(a) a uniform random key at the top of the kernel's static gate, (b) a key with a planted constant run that puts
the device-reported certified bound into [0.35, 0.5), (c) a fully crafted key at the smallest logB whose bound
reaches 1/2, which must be refused before any launch, and at the logB below it, which must be exact.

Collection stays free of the native library: the parameter lists are literals
(tests/test_keygen_abi.py::test_table_sweeps_are_complete_and_collect_without_the_library).
tests/test_worst_case_inputs.py checks on the CPU that the inputs are what they claim to be and that every
literal logB sits at the top of its gate.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import worst_case as W  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
WINDOW = (0.35, 0.5)   # leg (b): where the device-reported bound of the planted key must lie
TARGET = 0.44          # ... and where the run length aims

# (id, k, N, l, logB, top, options).  `top` says why logB is the largest the case can take
# (test_worst_case_inputs.py::test_every_logb_is_at_the_top_of_its_gate):
#   gate   the kernel's static gate (pbs.hpp) admits logB and not logB + 1
#   whole  l = 1, logB = 15: the last whole digit on the 16-bit limb grid (16 would split into sub-digits)
#   t2     the kernel instance is the one for two sub-digits: logB = 2 x limb bits
#   even   the library admits l (logB + 1) = 64, where no extreme word is even (worst_case.extreme_words)
#   flagship  the benchmark decompositions 3/7 (N = 1024) and 1/23 (N = 2048), one below their gates' tops
# options: env = CONCRETE_HIP_PBS_* overrides, route = "generic" (general-format key through
# concrete_hip_pbs_generic), words = "subdigit", batch = 3.
PBS_CASES = [
    # N1024 (k = 1): (k+1) l 2^logB <= 4096
    ("n1024-l1b11", 1, 1024, 1, 11, "gate", {}),
    ("n1024-l2b10", 1, 1024, 2, 10, "gate", {}),
    ("n1024-l3b9", 1, 1024, 3, 9, "gate", {}),
    ("n1024-l3b7", 1, 1024, 3, 7, "flagship", {}),
    ("n1024-l3b9-pairs1", 1, 1024, 3, 9, "gate", {"env": {"PAIRS": 1, "QUAD": 0}}),
    ("n1024-l3b9-pairs2", 1, 1024, 3, 9, "gate", {"env": {"PAIRS": 2, "QUAD": 0}}),
    ("n1024-l3b9-pairs4", 1, 1024, 3, 9, "gate", {"env": {"PAIRS": 4}}),
    ("n1024-l3b9-quad1", 1, 1024, 3, 9, "gate", {"env": {"QUAD": 1}}),
    ("n1024-l3b9-quad2", 1, 1024, 3, 9, "gate", {"env": {"QUAD": 2}}),
    ("n1024-l3b9-hex1", 1, 1024, 3, 9, "gate", {"env": {"HEX": 1}}),
    ("n1024-l3b9-hex2", 1, 1024, 3, 9, "gate", {"env": {"HEX": 2}}),
    ("n1024-l3b9-slot", 1, 1024, 3, 9, "gate", {"env": {"SLOT": 1}}),
    ("n1024-l3b7-slot", 1, 1024, 3, 7, "flagship", {"env": {"SLOT": 1}}),
    # N2048 (k = 1): l = 1 sub-digits up to 24 bits, l >= 2 whole digits with l 2^(logB-1) <= 2^15
    ("n2048-l1b24", 1, 2048, 1, 24, "gate", {}),
    ("n2048-l1b23-sub", 1, 2048, 1, 23, "flagship", {"words": "subdigit"}),
    ("n2048-l2b15", 1, 2048, 2, 15, "gate", {}),
    ("n2048-l3b14", 1, 2048, 3, 14, "gate", {}),
    ("n2048-l4b14", 1, 2048, 4, 14, "gate", {}),
    # K2N1024 (k = 2): l = 3 is the first level-major key, l = 5 the many-level kernel
    ("k2n1024-l1b24", 2, 1024, 1, 24, "gate", {}),
    ("k2n1024-l1b24-sub", 2, 1024, 1, 24, "gate", {"words": "subdigit"}),
    ("k2n1024-l2b15", 2, 1024, 2, 15, "gate", {}),
    ("k2n1024-l3b14", 2, 1024, 3, 14, "gate", {}),
    ("k2n1024-l5b12", 2, 1024, 5, 12, "gate", {}),
    # SMALL: 16-bit limbs, and 13-bit limbs at (4, 512, 2)
    ("k3n512-l1b24", 3, 512, 1, 24, "gate", {}),
    ("k3n512-l1b15", 3, 512, 1, 15, "whole", {}),
    ("k3n512-l2b15", 3, 512, 2, 15, "gate", {}),
    ("k3n512-l3b14", 3, 512, 3, 14, "gate", {}),
    ("k5n256-l1b24", 5, 256, 1, 24, "gate", {}),
    ("k5n256-l2b15", 5, 256, 2, 15, "gate", {}),
    ("k6n256-l1b24", 6, 256, 1, 24, "gate", {}),
    ("k6n256-l2b15", 6, 256, 2, 15, "gate", {}),
    ("k4n512-l1b24", 4, 512, 1, 24, "gate", {"words": "subdigit"}),
    ("k4n512-l2b16", 4, 512, 2, 16, "gate", {}),
    ("k4n512-l3b14", 4, 512, 3, 14, "gate", {}),
    ("k4n512-l6b10", 4, 512, 6, 10, "gate", {}),
    # GENERIC: one shape per route of pbs_generic.hip
    ("gen-tile-k2n1024", 2, 1024, 1, 26, "t2", {"route": "generic"}),
    ("gen-twolaunch-k3n1024", 3, 1024, 2, 26, "gate", {}),
    ("gen-fourstep-n2048-l5", 1, 2048, 5, 12, "gate", {}),
    ("gen-fused-n4096", 1, 4096, 1, 26, "gate", {}),
    ("gen-coop-n8192", 1, 8192, 1, 24, "t2", {}),
    ("gen-n16384", 1, 16384, 2, 31, "even", {}),
    ("gen-split-n32768", 1, 32768, 2, 31, "even", {"batch": 3}),
    ("gen-split-n65536", 1, 65536, 2, 30, "gate", {"batch": 3}),
    ("gen-companion-n1024-l3", 1, 1024, 3, 21, "gate", {"route": "generic"}),
]

# Legs that cannot be reached, by case id, with the reason; the test asserts both directions (a listed case
# must really miss the leg, an unlisted one must reach it).
#   BELOW_WINDOW: no run length reaches the window: the key with every polynomial of one GGSW at the
#   limb-extreme word (m = N) still has its bound below 0.35; leg (b) runs with that key.
BELOW_WINDOW = {
    "k4n512-l6b10": "six levels of 10-bit digits: the limb-extreme key's bound is 0.20",
    "gen-tile-k2n1024": "13-bit limbs under 26-bit digits, two sub-digits: the limb-extreme key's bound is 0.18",
}
#   NO_REFUSAL: no logB up to the case's own makes the fully crafted key's bound reach 1/2, with either word.
NO_REFUSAL = {
    "n1024-l3b7": "3/7 is two bits below the l = 3 gate: 0.45 with the limb-extreme key; n1024-l3b9 is refused from 8",
    "n1024-l3b7-slot": "as n1024-l3b7",
    "k4n512-l6b10": "the limb-extreme key's bound is 0.20 at the gate's top",
    "gen-tile-k2n1024": "the limb-extreme key's bound is 0.18 at logB = 26",
    "gen-twolaunch-k3n1024": "the limb-extreme key's bound is 0.49 at the gate's top",
    "gen-fourstep-n2048-l5": "the limb-extreme key's bound is 0.47 at the gate's top",
    "gen-companion-n1024-l3": "the limb-extreme key's bound is 0.36 at the gate's top",
}


def case_id(c):
    return c[0]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from concrete_amd import _native
    from concrete_amd import backend as B
    from oracle import pyoracle as O
    O.lib()
    return dict(torch=torch, L=_native.lib(), B=B, O=O, shape={})


def _filled(env, shape):
    t = env["torch"].empty(shape, dtype=env["torch"].int64, device=DEV)
    t.fill_(SENTINEL)  # below 2^63: the same bits as int64
    return t


class DeviceKey:
    """A standard key converted on the device by the case's route; rc is the conversion's return code."""

    def __init__(self, env, S, words):
        L, torch = env["L"], env["torch"]
        self.words = np.ascontiguousarray(words, dtype=np.uint64)
        size = (L.concrete_hip_generic_bsk_size_bytes if S.generic else L.concrete_hip_fourier_bsk_size_bytes)(
            S.n, S.k, S.l, S.N)
        assert size > 0
        self.t = torch.empty(size // 8, dtype=torch.int64, device=DEV)
        conv = L.concrete_hip_convert_bsk_generic if S.generic else L.concrete_hip_convert_bsk
        s = torch.cuda.current_stream(DEV).cuda_stream
        self.rc = conv(s, 0, self.t.data_ptr(), self.words.ctypes.data, 0, S.n, S.k, S.l, S.N)
        self.message = L.concrete_hip_last_error().decode(errors="replace") if self.rc else ""
        torch.cuda.synchronize()
        self.max_g = L.concrete_hip_key_spectrum_max(self.t.data_ptr())
        self._L = L

    def bound(self, logB):
        return self._L.concrete_hip_key_error_bound(self.t.data_ptr(), logB)


class Shape:
    """What the rows of one (k, N, l, logB, route, words, batch) share: parameters, batches, keys,
    conversions and oracle results, each made once."""

    def __init__(self, env, case):
        import ctypes as C
        _, self.k, self.N, self.l, self.logB, self.top, opts = case
        self.n = 2
        self.generic = opts.get("route") == "generic"
        self.words = opts.get("words", "extreme")
        self.batch = opts.get("batch", 9)
        L, B, O = env["L"], env["B"], env["O"]
        limbs, bits = C.c_uint32(), C.c_uint32()
        self.kind = L.concrete_hip_bsk_format(self.k, self.N, self.l, C.byref(limbs), C.byref(bits))
        self.limbs, self.bits = limbs.value, bits.value
        if self.generic:
            from oracle import keyref
            assert self.kind != keyref.KIND_GENERIC, "route=generic is for the companions of hand-tuned shapes"
            self.kind = keyref.KIND_GENERIC
            self.bits = keyref.generic_limb_bits(self.k, self.N, self.l)
            self.limbs = -(-64 // self.bits)
        self.widths = W.limb_widths(self.kind, self.limbs, self.bits)
        self.seed = 970000 + 7 * self.N + 131 * self.k + 17 * self.l + self.logB
        self.batches, self.refs, self.keys = {}, {}, {}

    def params(self, B, logB):
        return B.PbsParams(n=self.n, k=self.k, N=self.N, level=self.l, base_log=logB)

    def worst(self, env, logB, words):
        """The worst-case batch at logB on the host and on the device."""
        if (logB, words) not in self.batches:
            B = env["B"]
            cts, accs, lut_idx = W.worst_batch(self.k, self.N, self.l, logB, self.seed + logB, self.batch, words)
            self.batches[logB, words] = (cts, accs, lut_idx,
                                         tuple(B.to_device(a.copy(), DEV) for a in (cts, accs, lut_idx)))
        return self.batches[logB, words]

    def key(self, env, name, make):
        if name not in self.keys:
            self.keys[name] = DeviceKey(env, self, make())
        return self.keys[name]

    def ref(self, env, name, logB, words):
        """oracle.pbs_batch in Karatsuba mode on key `name` and the worst-case batch at logB."""
        if (name, logB, words) not in self.refs:
            O = env["O"]
            cts, accs, lut_idx, _ = self.worst(env, logB, words)
            op = O.Params(n=self.n, k=self.k, N=self.N, l=self.l, logB=logB)
            ref, _ = O.pbs_batch(op, cts, accs, bsk=self.keys[name].words, mode=O.MODE_KARATSUBA, lut_idx=lut_idx)
            ref.setflags(write=False)
            self.refs[name, logB, words] = ref
        return self.refs[name, logB, words]


def shape_of(env, case):
    """One shape at a time on the device: the override rows of a shape are neighbours in PBS_CASES."""
    ident = (case[1:5], tuple(sorted((k, v) for k, v in case[6].items() if k != "env")))
    if ident not in env["shape"]:
        env["shape"] = {ident: Shape(env, case)}
    return env["shape"][ident]


def run_pbs(env, S, key, logB, words):
    """One call on the worst-case batch at logB into the middle rows of a sentinel-filled tensor:
    (return code, message, the rows written, residual, whether both sentinel rows survived, every word of
    the written rows still a sentinel, device status)."""
    L, B, torch = env["L"], env["B"], env["torch"]
    _, _, _, (d_cts, d_accs, d_idx) = S.worst(env, logB, words)
    out = _filled(env, (S.batch + 2, S.k * S.N + 1))
    resid = torch.zeros(1, dtype=torch.int64, device=DEV)
    fn = L.concrete_hip_pbs_generic if S.generic else L.concrete_hip_pbs
    s = torch.cuda.current_stream(DEV).cuda_stream
    rc = fn(s, 0, out[1:].data_ptr(), None, d_accs.data_ptr(), d_idx.data_ptr(), d_cts.data_ptr(), None,
            key.t.data_ptr(), S.n, S.k, S.N, logB, S.l, S.batch, resid.data_ptr())
    msg = L.concrete_hip_last_error().decode(errors="replace") if rc else ""
    torch.cuda.synchronize()
    status = B.device_status(DEV)
    got = B.to_host(out)
    sentinel = np.uint64(SENTINEL)
    guards = bool((got[0] == sentinel).all() and (got[-1] == sentinel).all())
    untouched = bool((got[1:-1] == sentinel).all())
    return rc, msg, got[1:-1], float(B.to_host(resid).view(np.float64)[0]), guards, untouched, status


def check_exact(env, S, tag, name, logB, words):
    """The call runs, writes its rows only, leaves status 0, equals the oracle word for word, and its
    measured residual is below the bound the device reports for this key (the one-sided certificate)."""
    key = S.keys[name]
    bound = key.bound(logB)
    assert 0.0 < bound < 0.5, (tag, name, logB, bound)
    rc, msg, got, resid, guards, _, status = run_pbs(env, S, key, logB, words)
    assert rc == 0, (tag, name, logB, rc, msg)
    assert status == 0, (tag, name, logB, status)
    assert guards, f"{tag}: wrote outside its output rows"
    ref = S.ref(env, name, logB, words)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    print(f"{tag} key={name} logB={logB} batch={words}: max|G| {key.max_g:.4g}, bound {bound:.3e}, "
          f"residual {resid:.3e}")
    assert bad.size == 0, f"{tag} key={name} logB={logB}: rows {bad.tolist()} differ from the exact oracle"
    assert resid < bound, (tag, name, logB, resid, bound)
    return bound, resid


def check_refused(env, S, tag, key, logB, needle):
    """Refused with -2 before any launch: the message names the reason, the sentinel-filled output is
    untouched and the status is still 0."""
    rc, msg, _, _, guards, untouched, status = run_pbs(env, S, key, logB, "extreme")
    assert rc == -2, (tag, logB, rc, msg)
    assert needle in msg, (tag, logB, msg)
    assert guards and untouched, f"{tag}: a refused call wrote to its output"
    assert status == 0, (tag, logB, status)


def planted_run(S, key_a, bound_a):
    """Leg (b)'s planted run (word, m).  The bound is linear in max|G| apart from a small constant term, so the
    run aims at max|G| = max|G|_a TARGET / bound_a, with the 0x5555... word where its full run gets there and
    the format's limb-extreme word otherwise; where even that one's full run stays below the aim, m = N.  A
    random key that is already inside the window gets the shortest run, which leaves its max|G| where it is."""
    if bound_a >= WINDOW[0]:
        return W.CRAFTED, 1
    want = key_a.max_g * TARGET / bound_a
    for word in (W.CRAFTED, W.limb_extreme_word(S.widths)):
        m = W.run_for_spectrum(S.N, W.max_limb(word, S.widths), want)
        if m is not None:
            return word, m
    return W.limb_extreme_word(S.widths), S.N


@pytest.mark.parametrize("case", PBS_CASES, ids=case_id)
def test_pbs_worst_case(env, monkeypatch, case):
    tag, k, N, l, logB, top, opts = case
    L = env["L"]
    S = shape_of(env, case)
    for name, value in opts.get("env", {}).items():
        monkeypatch.setenv("CONCRETE_HIP_PBS_" + name, str(value))
    assert L.concrete_hip_pbs_supported(k, N, l, logB) == 1

    # (a) uniform random key, worst-case batch: the static gate's own claim
    key_a = S.key(env, "random", lambda: W.rand_u64(np.random.RandomState(S.seed), S.n * l * (k + 1) ** 2 * N))
    assert key_a.rc == 0, key_a.message
    bound_a, _ = check_exact(env, S, tag, "random", logB, S.words)
    check_exact(env, S, tag, "random", logB, "uniform")  # the figure the worst-case residuals are compared with
    if top == "gate" and l * (logB + 1) <= 63:
        # one past the gate the hand-tuned kernel does not run: a caller-held key has no general-format
        # companion, and the general path's own gate ends where concrete_hip_pbs_supported does
        check_refused(env, S, tag, key_a, logB + 1, "pbs")

    # (b) a planted run near the gate
    word, m = planted_run(S, key_a, bound_a)
    key_b = S.key(env, "near", lambda: W.crafted_key(k, N, l, S.n, 1, "alternating", m, word, S.seed + 1))
    assert key_b.rc == 0, key_b.message
    bound_b = key_b.bound(logB)
    print(f"{tag}: planted run m = {m} of {word:#x}: bound {bound_b:.3e}")
    if tag in BELOW_WINDOW:  # m = N of the limb-extreme word, and still below the window
        assert (word, m) == (W.limb_extreme_word(S.widths), N) and bound_b < WINDOW[0], (tag, hex(word), m, bound_b)
    else:
        assert WINDOW[0] <= bound_b < WINDOW[1], (tag, hex(word), m, bound_b)
    check_exact(env, S, tag, "near", logB, S.words)

    # (c) fully crafted key over the gate
    refuse = None
    for which, word in (("full", W.CRAFTED), ("full-extreme", W.limb_extreme_word(S.widths))):
        key_c = S.key(env, which, lambda: W.crafted_key(k, N, l, S.n, 0, "constant", N, word, S.seed + 2))
        if key_c.rc != 0:
            # the conversion itself refuses a key that no logB could use exactly (key_spectrum_record)
            assert key_c.rc == -2 and "certified rounding bound" in key_c.message, (key_c.rc, key_c.message)
            assert key_c.bound(1) >= 0.5
            print(f"{tag}: conversion refuses the {which} key (bound at logB = 1: {key_c.bound(1):.3f})")
            assert tag not in NO_REFUSAL
            return
        over = [b for b in range(1, logB + 1) if key_c.bound(b) >= 0.5]
        if over:
            refuse = over[0]
            break
    assert (refuse is None) == (tag in NO_REFUSAL), (tag, refuse, key_c.bound(logB))
    if refuse is None:
        print(f"{tag}: no logB <= {logB} is refused; bound of the limb-extreme key {key_c.bound(logB):.3e}")
        check_exact(env, S, tag, which, logB, "extreme")
        return
    print(f"{tag}: {which} key refused from logB = {refuse} (bound {key_c.bound(refuse):.3f})")
    check_refused(env, S, tag, key_c, refuse, "certified rounding bound")
    if refuse > 1:
        check_exact(env, S, tag, which, refuse - 1, "extreme")


# ---------------------------------------------------------------------------------------------------------
# keyswitch
# ---------------------------------------------------------------------------------------------------------
KS_VALU_BATCH = 11  # below KS_MFMA_MIN_BATCH = 64: the VALU kernel
# (l, logB, dmax = l 2^(logB-1), int32 chunk form: 3 chunks up to 32, 4 up to 1024, 0 = 64-bit products)
KS_VALU_CASES = [
    (1, 6, 32, 3), (2, 5, 32, 3), (4, 4, 32, 3), (32, 1, 32, 3), (1, 7, 64, 4),
    (1, 11, 1024, 4), (2, 10, 1024, 4), (4, 9, 1024, 4), (1, 12, 2048, 0),
]
# (n_in, n_out): 64 a whole and 100 a ragged int32 block, unsplit (n_in < 256); 292 splits in two
# (keyswitch.hip:keyswitch_launch); n_out + 1 = 200 and 631
KS_VALU_SHAPES = [(64, 199), (100, 630), (292, 199), (292, 630)]
KS_KEYS = ["ones", "i8min", "i8max", "uniform"]


def run_keyswitch(env, n_in, n_out, l, logB, cts, ksk):
    B, O, torch = env["B"], env["O"], env["torch"]
    batch = cts.shape[0]
    p = B.PbsParams(n=n_out, k=1, N=n_in, level=1, base_log=1, ks_level=l, ks_base_log=logB)
    out = _filled(env, (batch + 1, n_out + 1))
    B.keyswitch(p, B.to_device(ksk, DEV), B.to_device(cts.copy(), DEV), out=out, num_samples=batch)
    torch.cuda.synchronize()
    got = B.to_host(out)
    op = O.Params(n=n_out, k=1, N=n_in, l=1, logB=1, ks_l=l, ks_logB=logB)
    want = O.keyswitch_batch(op, cts, ksk)
    assert (got[batch] == np.uint64(SENTINEL)).all(), "wrote past the output"
    return got[:batch], want


@pytest.mark.parametrize("case", KS_VALU_CASES, ids=lambda c: "l%db%d" % c[:2])
def test_keyswitch_valu_worst_case(env, case):
    """The VALU kernel's int32 chunk forms exactly at dmax = 32 and 1024 and one past each, on rows of
    extreme digits against keys whose every chunk is at its maximum."""
    l, logB, dmax, nch = case
    assert dmax == l << (logB - 1)
    assert nch == (3 if dmax <= 32 else 4 if dmax <= 1024 else 0)
    for n_in, n_out in KS_VALU_SHAPES:
        cts = W.ks_inputs(n_in, l, logB, KS_VALU_BATCH, 1000 * l + logB + n_in)
        for name in KS_KEYS:
            ksk = W.ks_key(n_in, l, n_out, name, 77 + n_in)
            got, want = run_keyswitch(env, n_in, n_out, l, logB, cts, ksk)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, f"l={l} logB={logB} n_in={n_in} n_out={n_out} key={name}: rows {bad.tolist()} differ"


KS_MFMA_BATCH = 64  # KS_MFMA_MIN_BATCH: the matrix-core kernel where ks_mfma_ok admits the shape
# (n_in, l, logB, on the matrix cores): K = n_in l at the edge K 2^(logB-1) 128 <= 2^31 - 1 and one past it
KS_MFMA_CASES = [
    (87381, 3, 7, True),     # K = 262143
    (65536, 4, 7, False),    # K = 262144: falls to the VALU kernel
    (299593, 7, 4, True),    # K = 2097151
]


@pytest.mark.parametrize("case", KS_MFMA_CASES, ids=lambda c: "K%db%d" % (c[0] * c[1], c[2]))
def test_keyswitch_mfma_worst_case(env, case):
    """The int8 matrix-core kernel at the edge of its int32 accumulators (ks_mfma_ok), n_out = 7: every digit
    at its extreme against every balanced key byte at -128; one past the edge the VALU kernel takes the call."""
    n_in, l, logB, mfma = case
    K = n_in * l
    assert (K * (1 << (logB - 1)) * 128 <= 0x7FFFFFFF) == mfma and logB <= 7
    n_out = 7
    cts = W.ks_inputs(n_in, l, logB, KS_MFMA_BATCH, K)
    for name in ("i8min", "i8max"):
        ksk = W.ks_key(n_in, l, n_out, name, 0)
        got, want = run_keyswitch(env, n_in, n_out, l, logB, cts, ksk)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, f"K={K} logB={logB} key={name}: rows {bad.tolist()} differ from the oracle"
