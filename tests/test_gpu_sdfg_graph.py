"""GPU tests of the SDFG stream emulator's graph machinery (concrete_amd/csrc/sdfg.hip): every
process kind, sharding with a remainder and with fewer samples than device entries, chunked shards
(CONCRETE_HIP_SDFG_CHUNK_SAMPLES), fan-out, a stream used twice by one process, two bootstraps in
one subgraph, several downloaded streams, staleness by value and by count, two key sets, memref
descriptors with offsets and padded rows.

Every graph is built twice by one `Graph` object: on the device through concrete_amd.runtime.Dfg
and in `Model`, an eager host evaluator (numpy wrapping uint64 arithmetic for the four linear
operations as linear.hip's header states them, the oracle's keyswitch and PBS, backend.trivial_glwe
from a LUT row to an accumulator).  Every comparison is np.array_equal: no tolerances.

Run as a script (`test_gpu_sdfg_graph.py trace both|topo`) this file is the child process of
test_staleness_by_count: it replays the fan-out sequence so the parent can read the emulator's
trace from stderr.
"""
import os
import re
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS_X86_TO_TOPO, TS_TOPO_TO_TOPO, TS_TOPO_TO_X86, TS_TOPO_TO_BOTH = 0, 1, 2, 3
U64_MAX = (1 << 64) - 1
EDGE_SCALARS = [0, 1, 1 << 63, U64_MAX]
WIDTH = 2  # message bits of the encrypted graphs


# ---- the host model ------------------------------------------------------------------------------
def op_add(a, b):
    return a + b  # every word, wrapping


def op_add_pt(a, p):
    out = a.copy()
    out[:, -1] += p.reshape(-1)  # body word only; one value per sample or one for all
    return out


def op_mul(a, c):
    return a * c.reshape(-1, 1)  # every word


def op_neg(a):
    return np.zeros_like(a) - a  # every word


class Model:
    """Eager reference of a stream graph.  Values: a produced stream holds what its process makes of
    its inputs, unless a value put on it is newer than every put reaching its inputs.  Schedule: a
    get runs a process iff its output is stale or never reached the host, and copies back the
    target, the streams typed for the host and the streams a process outside the run consumes."""

    def __init__(self):
        self.procs = {}      # out -> (fn, input names)
        self.users = {}      # stream -> outputs of its consumers
        self.stype = {}
        self.puts = {}       # stream -> (clock, value)
        self.clock = 0
        self.memo = {}
        self.done = {}       # produced stream -> eff it was computed for
        self.host = set()    # produced streams whose value is on the host

    def proc(self, out, fn, *ins):
        self.procs[out] = (fn, ins)
        for i in ins:
            self.users.setdefault(i, []).append(out)

    def put(self, name, value=None):
        self.clock += 1
        self.puts[name] = (self.clock, None if value is None else np.array(value, dtype=np.uint64))
        if name in self.procs:
            self.done[name] = self.eff(name)
            self.host.add(name)

    def eff(self, name):
        v = self.puts.get(name, (0, None))[0]
        if name in self.procs:
            v = max([v] + [self.eff(i) for i in self.procs[name][1]])
        return v

    def value(self, name):
        if name not in self.procs:
            return self.puts[name][1]
        fn, ins = self.procs[name]
        if name in self.puts and self.puts[name][0] > max(self.eff(i) for i in ins):
            return self.puts[name][1]
        key = (name, self.eff(name))
        if key not in self.memo:
            self.memo[key] = fn(*[self.value(i) for i in ins])
        return self.memo[key]

    def get(self, target):
        """(processes run, in order; streams copied back) of a get of `target`."""
        q = []

        def need(s):
            if s not in self.procs or s in q:
                return
            if self.done.get(s) == self.eff(s) and s in self.host:
                return
            for i in self.procs[s][1]:
                need(i)
            q.append(s)

        need(target)
        down = {s for s in q if s == target or self.stype[s] in (TS_TOPO_TO_X86, TS_TOPO_TO_BOTH)
                or any(c not in q for c in self.users.get(s, []))}
        for s in q:
            self.done[s] = self.eff(s)
            (self.host.add if s in down else self.host.discard)(s)
        return q, down


class Graph:
    """One graph, built on the device (when `R` is given) and in the model, stream by name."""

    def __init__(self, R=None):
        self.R = R
        self.g = R.Dfg() if R else None
        self.m = Model()
        self.h = {}

    def stream(self, name, kind="batch", stype=TS_TOPO_TO_TOPO):
        self.m.stype[name] = stype
        if self.g:
            make = {"batch": self.g.batch_stream, "memref": self.g.memref_stream, "u64": self.g.uint64_stream}[kind]
            self.h[name] = make(name, stype)
        return name

    def inputs(self, *names, kind="batch"):
        for n in names:
            self.stream(n, kind, TS_X86_TO_TOPO)

    def linear(self, op, a, b, out):
        fn = {"add": op_add, "add_pt": op_add_pt, "add_pt_cst": op_add_pt, "mul": op_mul, "mul_cst": op_mul,
              "neg": op_neg}[op]
        self.m.proc(out, fn, *([a] if op == "neg" else [a, b]))
        if self.g:
            self.g.linear(op, self.h[a], None if op == "neg" else self.h[b], self.h[out])

    def keyswitch(self, a, out, K, index=0):
        self.m.proc(out, K and K.keyswitch, a)
        if self.g:
            self.g.keyswitch(self.h[a], self.h[out], K.pks, K.ctx, ksk_index=index)

    def bootstrap(self, a, lut, out, K, index=0, mapped=False):
        self.m.proc(out, K and K.bootstrap, a, lut)
        if self.g:
            self.g.bootstrap(self.h[a], self.h[lut], self.h[out], K.p, K.ctx, bsk_index=index, mapped=mapped)

    def put(self, name, value):
        """A 2-D value goes as a batch, a 1-D one as a memref, an int as a uint64."""
        if isinstance(value, int):
            self.m.put(name, [value])
            if self.g:
                self.g.put_uint64(self.h[name], value)
            return
        self.m.put(name, value)
        if self.g:
            (self.g.put_batch if value.ndim == 2 else self.g.put_memref)(self.h[name], value)

    def fetch(self, name):
        want = self.m.value(name)
        self.m.get(name)
        return self.g.get_batch(self.h[name], *want.shape), want

    def check(self, name):
        got, want = self.fetch(name)
        assert np.array_equal(got, want), f"stream {name}: {int((got != want).sum())} of {want.size} words differ, " \
                                          f"rows {sorted({int(r) for r in np.nonzero(got != want)[0]})}"
        return got

    def close(self):
        if self.g:
            self.g.close()


# ---- keys ----------------------------------------------------------------------------------------
class Keys:
    """One key set: keyswitch big -> n and bootstrap (n, k, N), with the oracle's functions of them.
    `p` is the bootstrap's parameter set; `pks` carries the keyswitch's dimensions (its big_n is the
    keyswitch input, which need not be this bootstrap's output)."""

    def __init__(self, p, pks, sk_in, seed, karatsuba, ctx=None):
        from concrete_amd import backend as B
        from oracle import pyoracle as O
        self.B, self.O, self.p, self.pks, self.ctx = B, O, p, pks, ctx
        self.lwe_sk = B.binary_key(p.n, seed)
        self.glwe_sk = B.binary_key(p.big_n, seed + 1)
        self.bsk = B.bsk_generate(p, self.lwe_sk, self.glwe_sk, seed + 2)
        self.ksk = B.ksk_generate(pks, sk_in if sk_in is not None else self.glwe_sk, self.lwe_sk, seed + 3,
                                  std=2.0 ** -40)
        self.oks = O.Params(n=pks.n, k=pks.k, N=pks.N, l=1, logB=1, ks_l=pks.ks_level, ks_logB=pks.ks_base_log)
        self.op = O.Params(n=p.n, k=p.k, N=p.N, l=p.level, logB=p.base_log)
        # the oracle product that is bit-exact for this shape's kernel (tests/test_gpu_pbs_small.py,
        # tests/test_gpu_runtime.py)
        self.fcpu = None if karatsuba else O.bsk_to_fourier(self.op, self.bsk)

    def keyswitch(self, x):
        return self.O.keyswitch_batch(self.oks, x, self.ksk)

    def bootstrap(self, x, luts):
        accs = np.stack([self.B.trivial_glwe(self.p, row) for row in np.atleast_2d(luts)])
        idx = np.arange(len(x), dtype=np.uint64) if len(accs) > 1 else None
        if self.fcpu is None:
            return self.O.pbs_batch(self.op, x, accs, bsk=self.bsk, mode=self.O.MODE_KARATSUBA, lut_idx=idx)[0]
        return self.O.pbs_batch(self.op, x, accs, fbsk=self.fcpu, lut_idx=idx)[0]

    def lut(self, table):
        return self.B.expand_lut(np.asarray(table, dtype=np.uint64), self.p.N, WIDTH)

    def decode(self, cts):
        return [self.B.decode(d, WIDTH) for d in self.B.lwe_decrypt(self.glwe_sk, cts, self.p.big_n)]


def keys0(ctx=None):
    """N = 1024, k = 1 (the pair / quad kernel), n = 24; keyswitch 1024 -> 24."""
    from concrete_amd import backend as B
    p = replace(B.CFG2, n=24)
    return Keys(p, p, None, 4100, karatsuba=False, ctx=ctx)


def keys1(k0, ctx=None):
    """N = 512, k = 3, l = 1, logB = 18 (pbs_small.hip), n = 14; keyswitch 1024 -> 14 from key set 0's
    bootstrap output, with another level count and base than key set 0's."""
    from concrete_amd import backend as B
    p = replace(B.OPTIMIZER_SETS[3], n=14)
    pks = B.PbsParams(n=p.n, k=1, N=1024, level=p.level, base_log=p.base_log, ks_level=3, ks_base_log=4)
    assert pks.big_n == k0.p.big_n and (pks.ks_level, pks.ks_base_log) != (k0.pks.ks_level, k0.pks.ks_base_log)
    return Keys(p, pks, k0.glwe_sk, 4200, karatsuba=True, ctx=ctx)


CTX = 0x5DF6  # the runtime-context pointer the keyset is bound to


@pytest.fixture(scope="module")
def R():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from concrete_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def keysets(R):
    """Both key sets, generated once and registered at index 0 and 1 of one keyset."""
    k0 = keys0(CTX)
    k1 = keys1(k0, CTX)
    kset = R.Keyset([0])
    kset.add_bsk(0, k0.bsk, k0.p)
    kset.add_ksk(0, k0.ksk, k0.pks)
    kset.add_bsk(1, k1.bsk, k1.p)
    kset.add_ksk(1, k1.ksk, k1.pks)
    kset.bind(CTX)
    yield k0, k1
    kset.close()


def set_devices(monkeypatch, devices):
    """stream_emulator_init reads the list: call before constructing a Graph."""
    if devices:
        monkeypatch.setenv("CONCRETE_HIP_SDFG_DEVICES", devices)
    else:
        monkeypatch.delenv("CONCRETE_HIP_SDFG_DEVICES", raising=False)


def encrypt(K, sk, msgs, seed):
    return K.B.lwe_encrypt(sk, [K.B.encode(m, WIDTH) for m in msgs], len(sk), 2.0 ** -40, seed)


def words(rng, *shape):
    """Uniform over the whole uint64 range."""
    return rng.randint(0, 1 << 32, size=shape).astype(np.uint64) << np.uint64(32) | \
        rng.randint(0, 1 << 32, size=shape).astype(np.uint64)


# ---- 1. every linear process -----------------------------------------------------------------------
@pytest.mark.parametrize("form", ["memref", "batch"])
@pytest.mark.parametrize("devices", [None, "0,0,0"])
@pytest.mark.parametrize("width", [2, 631])
@pytest.mark.parametrize("batch", [1, 2, 7])
def test_every_linear_process(R, monkeypatch, batch, width, devices, form):
    """add -> add_pt(per sample) -> mul(per sample) -> mul_cst -> add_pt_cst -> neg on full-range
    words.  On "0,0,0" batch 7 is cut 3/2/2 and batch 2 uses two of the three entries.  The last
    stream, a device-only intermediate (recomputed) and a host-typed intermediate (reused) are read;
    then only the two constants are put again, over 0, 1, 2^63 and 2^64 - 1."""
    set_devices(monkeypatch, devices)
    rng = np.random.RandomState(1000 * batch + width)
    G = Graph(R)
    try:
        G.inputs("x", "y")
        G.inputs("pvec", "cvec", kind=form)
        G.inputs("c", "p", kind="u64")
        G.stream("s1")
        G.stream("s2", stype=TS_TOPO_TO_BOTH)
        G.stream("s3")
        G.stream("s4")
        G.stream("s5")
        G.stream("out", stype=TS_TOPO_TO_X86)
        G.linear("add", "x", "y", "s1")
        G.linear("add_pt", "s1", "pvec", "s2")
        G.linear("mul", "s2", "cvec", "s3")
        G.linear("mul_cst", "s3", "c", "s4")
        G.linear("add_pt_cst", "s4", "p", "s5")
        G.linear("neg", "s5", None, "out")
        G.g.run()
        x, y = words(rng, batch, width), words(rng, batch, width)
        x[0, 0], y[0, 0] = U64_MAX, 1  # a sum that wraps to 0
        pvec = words(rng, batch)
        cvec = np.array(([U64_MAX, 1 << 63] + [int(v) for v in words(rng, 3)] + [1, 0])[:batch], dtype=np.uint64)
        shape = (batch,) if form == "memref" else (batch, 1)
        G.put("x", x)
        G.put("y", y)
        G.put("pvec", pvec.reshape(shape))
        G.put("cvec", cvec.reshape(shape))
        G.put("c", int(words(rng, 1)[0]) | 1)
        G.put("p", int(words(rng, 1)[0]))
        want = op_neg(op_add_pt(op_mul(op_mul(op_add_pt(x + y, pvec), cvec), G.m.value("c")), G.m.value("p")))
        assert np.array_equal(G.m.value("out"), want)  # the model against the chain written out
        G.check("out")
        G.check("s3")   # device only after the first get: recomputed
        G.check("s2")   # typed for the host too: reused
        G.check("out")
        for c, p in zip(EDGE_SCALARS, EDGE_SCALARS[::-1]):
            G.put("c", c)
            G.check("out")
            G.put("p", p)
            G.check("out")
    finally:
        G.close()


@pytest.mark.parametrize("devices", [None, "0,0,0"])
def test_stream_used_twice_and_uint64_round_trip(R, monkeypatch, devices):
    """add(x, x): one stream as both operands of a process is uploaded once and read twice.  A value
    put on a uint64 stream reads back through get_uint64."""
    set_devices(monkeypatch, devices)
    rng = np.random.RandomState(7)
    G = Graph(R)
    try:
        G.inputs("x")
        G.inputs("v", kind="u64")
        G.stream("z")
        G.stream("w", stype=TS_TOPO_TO_X86)
        G.linear("add", "x", "x", "z")
        G.linear("mul_cst", "z", "v", "w")
        x = words(rng, 7, 5)
        x[3] = 1 << 63  # doubles to 0
        G.put("x", x)
        for v in EDGE_SCALARS + [0x0123456789ABCDEF]:
            G.put("v", v)
            assert G.g.get_uint64(G.h["v"]) == v
            got = G.check("w")
            assert np.array_equal(got, (x + x) * np.uint64(v))
        G.check("z")
    finally:
        G.close()


# ---- 2, 3. fan-out with two bootstraps, staleness by value ----------------------------------------------
def fanout(G, K, host_typed=()):
    """x -> KS -> s;  s -> PBS(one LUT) -> a;  s -> mapped PBS(one LUT row per sample) -> b;
    add(a, b) -> c;  neg(c) -> d.  Streams in `host_typed` are TOPO_TO_BOTH."""
    G.inputs("x", "luts")
    G.inputs("lut", kind="memref")
    for name in ("s", "a", "b", "c"):
        G.stream(name, stype=TS_TOPO_TO_BOTH if name in host_typed else TS_TOPO_TO_TOPO)
    G.stream("d", stype=TS_TOPO_TO_X86)
    G.keyswitch("x", "s", K)
    G.bootstrap("s", "lut", "a", K)
    G.bootstrap("s", "luts", "b", K, mapped=True)
    G.linear("add", "a", "b", "c")
    G.linear("neg", "c", None, "d")


def fanout_data(K, batch, seed):
    rng = np.random.RandomState(seed)
    msgs = rng.randint(0, 1 << WIDTH, size=batch)
    tables = rng.randint(0, 1 << WIDTH, size=(batch + 1, 1 << WIDTH))
    return dict(msgs=msgs, tables=tables, x=encrypt(K, K.glwe_sk, msgs, seed + 1),
                lut=K.lut(tables[0]), luts=np.stack([K.lut(t) for t in tables[1:]]))


def fanout_meaning(K, d, msgs, t0, tables):
    """d = -(lut(m) + luts[i](m)), on the message's width + 1 bits."""
    m8 = 1 << (WIDTH + 1)
    return K.decode(d) == [(-(int(t0[m]) + int(tables[i][m]))) % m8 for i, m in enumerate(msgs)]


@pytest.mark.parametrize("devices,batch", [(None, 7), ("0,0,0", 7), (None, 1), ("0,0,0", 2), (None, 10)])
def test_fanout_two_bootstraps(R, keysets, monkeypatch, devices, batch):
    """One keyswitch output feeds a broadcast-LUT and a mapped-LUT bootstrap of one subgraph; d, then
    a, then b are read, each bit-exact."""
    K = keysets[0]
    set_devices(monkeypatch, devices)
    D = fanout_data(K, batch, 300 + batch)
    G = Graph(R)
    try:
        fanout(G, K)
        for name in ("x", "lut", "luts"):
            G.put(name, D[name])
        d = G.check("d")
        assert fanout_meaning(K, d, D["msgs"], D["tables"][0], D["tables"][1:])
        a = G.check("a")
        assert K.decode(a) == [int(D["tables"][0][m]) for m in D["msgs"]]
        b = G.check("b")
        assert K.decode(b) == [int(D["tables"][1 + i][m]) for i, m in enumerate(D["msgs"])]
    finally:
        G.close()


@pytest.mark.parametrize("devices", [None, "0,0,0"])
def test_staleness_by_value(R, keysets, monkeypatch, devices):
    """Puts after the first get, each followed by a get compared with the model re-evaluated from the
    same sequence of puts: only the mapped LUTs, only x, a value on the intermediate s (used), x
    again (the value on s is overridden), only the broadcast LUT, and a read twice."""
    K = keysets[0]
    set_devices(monkeypatch, devices)
    batch = 7
    D, D2, D3 = (fanout_data(K, batch, seed) for seed in (400, 410, 420))
    G = Graph(R)
    try:
        fanout(G, K)
        for name in ("x", "lut", "luts"):
            G.put(name, D[name])
        first = G.check("d").copy()
        G.put("luts", D2["luts"])                       # 1. only the mapped LUTs
        d = G.check("d")
        assert fanout_meaning(K, d, D["msgs"], D["tables"][0], D2["tables"][1:]) and not np.array_equal(d, first)
        G.put("x", D2["x"])                             # 2. only x
        d = G.check("d")
        assert fanout_meaning(K, d, D2["msgs"], D["tables"][0], D2["tables"][1:])
        G.put("s", K.keyswitch(D3["x"]))                # 3. a value on the intermediate: used
        d = G.check("d")
        assert fanout_meaning(K, d, D3["msgs"], D["tables"][0], D2["tables"][1:])
        G.put("x", D["x"])                              # 4. x again: overrides the value on s
        d = G.check("d")
        assert fanout_meaning(K, d, D["msgs"], D["tables"][0], D2["tables"][1:])
        G.check("s")
        G.put("lut", D3["lut"])                         # only the broadcast LUT
        d = G.check("d")
        assert fanout_meaning(K, d, D["msgs"], D3["tables"][0], D2["tables"][1:])
        a1 = G.check("a").copy()                        # 5. twice in a row
        a2 = G.check("a")
        assert np.array_equal(a1, a2)
        G.check("b")
        G.check("d")
    finally:
        G.close()


# ---- 4. staleness by count -----------------------------------------------------------------------------
TRACE_BATCH, TRACE_CHUNK = 7, 3


def trace_sequence(G, K=None):
    """The puts and gets of the trace child; returns what the model schedules for every get."""
    D = [fanout_data(K, TRACE_BATCH, seed) for seed in (500, 510)] if K else None
    runs = []

    def put(name, i):
        if K:
            G.put(name, D[i][name])
        else:
            G.m.put(name)

    def get(name):
        if K:
            G.g.get_batch(G.h[name], TRACE_BATCH, K.p.big_n + 1 if name != "s" else K.p.n + 1)
        runs.append((name,) + G.m.get(name))

    for name in ("x", "lut", "luts"):
        put(name, 0)
    get("d")
    put("luts", 1)   # only the mapped bootstrap's LUTs change
    get("d")
    get("a")
    get("b")
    put("x", 1)
    get("d")
    return runs


@pytest.mark.parametrize("mode", ["both", "topo"])
def test_staleness_by_count(mode):
    """The emulator's trace in a child process against the model's schedule: a process reruns iff its
    output is stale or never reached the host.  With s and a typed TOPO_TO_BOTH, new mapped LUTs
    rerun neither the keyswitch nor the first bootstrap (b needs s, so s is host-typed too); with
    every intermediate TOPO_TO_TOPO they rerun both.  The child runs one device entry with 3 samples
    per chunk: each get that runs anything runs ceil(7 / 3) chunks."""
    env = dict(os.environ, CONCRETE_HIP_SDFG_TRACE="1", CONCRETE_HIP_SDFG_DEVICES="0",
               CONCRETE_HIP_SDFG_CHUNK_SAMPLES=str(TRACE_CHUNK))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "trace", mode], env=env, capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "trace child ok" in res.stdout
    G = Graph()
    fanout(G, None, host_typed=("s", "a") if mode == "both" else ())
    want = trace_sequence(G)
    gets = []  # (target, outputs of the processes run, the downloaded ones)
    for line in res.stderr.splitlines():
        m = re.match(r"\[sdfg\] get (\w+): (\d+) processes, batch (\d+), (\d+) devices:(.*)", line)
        if m:
            # (a get that runs nothing plans no inputs and reports batch 1)
            assert (int(m.group(3)), int(m.group(4))) == (TRACE_BATCH if int(m.group(2)) else 1, 1), line
            outs = re.findall(r" \d+->(\w+?)(\(D2H\))?(?= |$)", m.group(5))
            assert len(outs) == int(m.group(2)), line
            gets.append((m.group(1), [o for o, _ in outs], {o for o, d in outs if d}))
    assert [g[0] for g in gets] == [w[0] for w in want] == ["d", "d", "a", "b", "d"]
    for got, (name, q, down) in zip(gets, want):
        assert got[1] == q and got[2] == down, (mode, name, got, q, down)
    counts = [len(g[1]) for g in gets]
    assert counts == ([5, 3, 0, 1, 5] if mode == "both" else [5, 5, 2, 1, 5]), counts
    if mode == "both":
        assert gets[1][1] == ["b", "c", "d"]  # neither the keyswitch nor the first bootstrap
    else:
        assert gets[1][1][:2] == ["s", "a"] and gets[2][2] == {"s", "a"}
    chunks = chunk_counts(res.stderr)
    assert chunks == [-(-TRACE_BATCH // TRACE_CHUNK) if n else 0 for n in counts], chunks


def chunk_counts(stderr):
    """Chunks run by every get: the trace prints the subgraph's inputs once per chunk."""
    counts, first = [], None
    for line in stderr.splitlines():
        if line.startswith("[sdfg] get "):
            counts.append(0)
            first = None
        m = re.match(r"\[sdfg\]   input (\w+) ", line)
        if m:
            first = first or m.group(1)
            counts[-1] += m.group(1) == first
    return counts


def trace_child(mode):
    from concrete_amd import runtime as R
    K = keys0(CTX)
    kset = R.Keyset([0])
    kset.add_bsk(0, K.bsk, K.p)
    kset.add_ksk(0, K.ksk, K.pks)
    kset.bind(CTX)
    G = Graph(R)
    fanout(G, K, host_typed=("s", "a") if mode == "both" else ())
    trace_sequence(G, K)
    G.close()
    kset.close()
    print("trace child ok")


# ---- 5. chunking -------------------------------------------------------------------------------------
def test_chunked_shards(R, keysets, monkeypatch):
    """Batch 10 on "0,0" (shards 5/5) with 3 samples per chunk (3 + 2 each), with 1 and with more
    than a shard: a broadcast scalar, a per-sample plaintext, a broadcast-LUT and a mapped-LUT
    bootstrap, a host-typed intermediate and the target downloaded.  Equal to the model, so to each
    other."""
    K = keysets[0]
    batch = 10
    set_devices(monkeypatch, "0,0")
    rng = np.random.RandomState(600)
    msgs = rng.randint(0, 2, size=batch)
    pbits = rng.randint(0, 2, size=batch)
    tables = rng.randint(0, 1 << WIDTH, size=(batch + 1, 1 << WIDTH))
    x = encrypt(K, K.glwe_sk, msgs, 601)
    results = []
    for chunk in ("3", "1", "64"):
        monkeypatch.setenv("CONCRETE_HIP_SDFG_CHUNK_SAMPLES", chunk)
        G = Graph(R)
        try:
            G.inputs("x", "luts")
            G.inputs("pvec", "lut", kind="memref")
            G.inputs("one", kind="u64")
            for name in ("x1", "x2", "s", "b"):
                G.stream(name)
            G.stream("a", stype=TS_TOPO_TO_BOTH)
            G.stream("c", stype=TS_TOPO_TO_X86)
            G.linear("add_pt_cst", "x", "one", "x1")
            G.linear("add_pt", "x1", "pvec", "x2")
            G.keyswitch("x2", "s", K)
            G.bootstrap("s", "lut", "a", K)
            G.bootstrap("s", "luts", "b", K, mapped=True)
            G.linear("add", "a", "b", "c")
            G.put("x", x)
            G.put("one", int(K.B.encode(1, WIDTH)))
            G.put("pvec", np.array([K.B.encode(v, WIDTH) for v in pbits], dtype=np.uint64))
            G.put("lut", K.lut(tables[0]))
            G.put("luts", np.stack([K.lut(t) for t in tables[1:]]))
            c = G.check("c").copy()
            a = G.check("a").copy()  # downloaded by the same run
            results.append((c, a))
        finally:
            G.close()
    m = msgs + 1 + pbits
    assert K.decode(results[0][1]) == [int(tables[0][v]) for v in m]
    assert K.decode(results[0][0]) == [(int(tables[0][v]) + int(tables[1 + i][v])) % 8 for i, v in enumerate(m)]
    for c, a in results[1:]:
        assert np.array_equal(c, results[0][0]) and np.array_equal(a, results[0][1])


# ---- 6. two key sets in one graph ------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, "0,0"])
@pytest.mark.parametrize("batch", [1, 7])
def test_two_key_sets(R, keysets, monkeypatch, devices, batch):
    """x -> KS[0] -> PBS[0] (N = 1024, k = 1) -> KS[1] (1024 -> 14) -> PBS[1] (N = 512, k = 3): keys of
    different shapes at index 0 and 1, every stage host-typed and bit-exact against the oracle."""
    K0, K1 = keysets
    set_devices(monkeypatch, devices)
    rng = np.random.RandomState(700 + batch)
    msgs = rng.randint(0, 1 << WIDTH, size=batch)
    t0, t1 = rng.permutation(1 << WIDTH), rng.permutation(1 << WIDTH)
    G = Graph(R)
    try:
        G.inputs("x")
        G.inputs("lut0", "lut1", kind="memref")
        for name in ("s0", "a0", "s1"):
            G.stream(name, stype=TS_TOPO_TO_BOTH)
        G.stream("r", stype=TS_TOPO_TO_X86)
        G.keyswitch("x", "s0", K0, index=0)
        G.bootstrap("s0", "lut0", "a0", K0, index=0)
        G.keyswitch("a0", "s1", K1, index=1)
        G.bootstrap("s1", "lut1", "r", K1, index=1)
        G.put("x", encrypt(K0, K0.glwe_sk, msgs, 701))
        G.put("lut0", K0.lut(t0))
        G.put("lut1", K1.lut(t1))
        r = G.check("r")
        assert r.shape == (batch, 3 * 512 + 1)
        assert K1.decode(r) == [int(t1[t0[m]]) for m in msgs]
        for name in ("s0", "a0", "s1"):
            G.check(name)
        assert K0.decode(G.m.value("a0")) == [int(t0[m]) for m in msgs]
    finally:
        G.close()


# ---- 7. memref descriptors -------------------------------------------------------------------------------
def test_descriptors_with_offsets_and_padded_rows(R, monkeypatch):
    """put_memref_batch from inside a larger array (offset 5, row stride cols + 3), get_memref_batch
    into a sentinel-filled array (offset 7, row stride cols + 4): every payload word matches, every
    other word keeps the sentinel.  get_memref reads a one-row batch stream."""
    set_devices(monkeypatch, None)
    rng = np.random.RandomState(800)
    rows, cols = 7, 5
    SENT = np.uint64(0xA5A5A5A5DEADBEEF)
    backing = words(rng, 5 + rows * (cols + 3) + 11)
    x = np.stack([backing[5 + r * (cols + 3): 5 + r * (cols + 3) + cols] for r in range(rows)])
    g = R.Dfg()
    try:
        sx = g.batch_stream("x", TS_X86_TO_TOPO)
        sy = g.batch_stream("y", TS_TOPO_TO_X86)
        g.linear("neg", sx, None, sy)
        g.lib.stream_emulator_put_memref_batch(sx, backing.ctypes.data, backing.ctypes.data, 5, rows, cols, cols + 3,
                                               1, 0)
        out = np.full(7 + rows * (cols + 4) + 9, SENT, dtype=np.uint64)
        g.lib.stream_emulator_get_memref_batch(sy, out.ctypes.data, out.ctypes.data, 7, rows, cols, cols + 4, 1)
        payload = np.zeros(out.shape, dtype=bool)
        for r in range(rows):
            payload[7 + r * (cols + 4): 7 + r * (cols + 4) + cols] = True
        assert np.array_equal(out[payload].reshape(rows, cols), op_neg(x))
        assert np.all(out[~payload] == SENT)
        assert np.array_equal(g.get_batch(sy, rows, cols), op_neg(x))  # the dense form of the same stream
        # the put stream itself, through the padded output descriptor
        out[:] = SENT
        g.lib.stream_emulator_get_memref_batch(sx, out.ctypes.data, out.ctypes.data, 7, rows, cols, cols + 4, 1)
        assert np.array_equal(out[payload].reshape(rows, cols), x) and np.all(out[~payload] == SENT)
        # one row: a batch stream read as a memref, at an offset
        g.put_batch(sx, x[2:3])
        one = np.full(cols + 6, SENT, dtype=np.uint64)
        g.lib.stream_emulator_get_memref(sy, one.ctypes.data, one.ctypes.data, 4, cols, 1)
        assert np.array_equal(one[4:4 + cols], op_neg(x[2])) and np.all(one[:4] == SENT) and np.all(one[-2:] == SENT)
        assert np.array_equal(g.get_memref(sy, cols), op_neg(x[2]))
        # a memref put at an offset
        sm = g.memref_stream("m", TS_X86_TO_TOPO)
        g.lib.stream_emulator_put_memref(sm, backing.ctypes.data, backing.ctypes.data, 9, 6, 1, 0)
        assert np.array_equal(g.get_memref(sm, 6), backing[9:15])
    finally:
        g.close()


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    assert len(sys.argv) == 3 and sys.argv[1] == "trace" and sys.argv[2] in ("both", "topo"), sys.argv
    trace_child(sys.argv[2])
