"""Difference two hipcc -S device listings of the same file (a refactor's before / after).

  python tools/isa_diff.py OLD.s NEW.s

Per kernel symbol: VGPR, AGPR, spill counts and the LDS / scratch sizes of the kernel metadata.
Per file: the opcode histogram, split into the opcodes that must match (vector, LDS, memory,
s_waitcnt / s_barrier / s_sleep / s_nop) and the rest (scalar ALU, branches).  Exit status 1 when
a register count, a size or a must-match opcode differs."""
import collections, re, sys

MUST = ("v_", "ds_", "global_", "buffer_", "flat_", "scratch_", "s_waitcnt", "s_barrier", "s_sleep", "s_nop")
FIELDS = ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size")


def kernels(text):
    out = {}
    for blk in re.split(r"\n  - (?=\.agpr_count:)", text)[1:]:
        blk = blk.split("\namdhsa.target")[0]
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in FIELDS)
    return out


def histogram(text, per_kernel):
    cnt, name = collections.Counter(), None
    for l in text.split(".amdgpu_metadata")[0].split("\n"):
        s = l.split(";")[0].strip()
        if s.startswith("_Z") and s.endswith(":"):
            name = s[:-1]
        elif s and not s.startswith(".") and not s.endswith(":"):
            cnt[s.split()[0]] += 1
            if s.startswith(MUST):
                per_kernel[name][s.split()[0]] += 1
    return cnt


old, new = open(sys.argv[1]).read(), open(sys.argv[2]).read()
ko, kn = kernels(old), kernels(new)
bad = 0
for name in sorted(set(ko) | set(kn)):
    if ko.get(name) != kn.get(name):
        bad += 1
        print("KERNEL", name, dict(zip(FIELDS, ko.get(name, ()))), "->", dict(zip(FIELDS, kn.get(name, ()))))
po, pn = collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
ho, hn = histogram(old, po), histogram(new, pn)
for name in sorted(kn):
    if po[name] != pn[name]:
        print("MIX   ", name, {m: (po[name][m], pn[name][m]) for m in set(po[name]) | set(pn[name])
                               if po[name][m] != pn[name][m]})
must = {m: (ho[m], hn[m]) for m in sorted(set(ho) | set(hn)) if ho[m] != hn[m] and m.startswith(MUST)}
free = {m: (ho[m], hn[m]) for m in sorted(set(ho) | set(hn)) if ho[m] != hn[m] and not m.startswith(MUST)}
for m, (a, b) in must.items():
    print(f"MUST-MATCH {m}: {a} -> {b}")
for m, (a, b) in free.items():
    print(f"scalar     {m}: {a} -> {b}")
print(f"{len(kn)} kernels, {bad} with other registers/sizes; {sum(ho.values())} -> {sum(hn.values())} instructions, "
      f"{len(must)} must-match opcodes differ, {len(free)} scalar opcodes differ")
sys.exit(1 if bad or must or set(ko) != set(kn) else 0)
