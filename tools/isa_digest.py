"""Digest of every kernel's instruction stream in gfx950 assembly listings (hipcc -S --cuda-device-only with the flags of build.py).

    python tools/isa_digest.py <file.s>                  one line per kernel
    python tools/isa_digest.py <parent.s> <child.s>      both, paired, and whether every kernel kept its stream

Per kernel: the demangled name, the instruction count, the register / scratch / LDS / occupancy lines of the listing and a SHA-256 of
the normalised instruction stream: comments and assembler directives dropped, white space folded, .LBB<function>_<block> labels
renumbered without the function's number and mangled symbols replaced by a placeholder -- so a kernel whose template-argument list
shrank, or that moved inside its file, keeps its digest exactly when it kept its instructions.  Kernels are paired by function name
(without template arguments) and digest: a refactor passes when every name has the same multiset of (digest, metadata) on both sides.
The tool compares listings; it knows nothing about particular instructions."""
import collections
import hashlib
import re
import subprocess
import sys

META = ("NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels_of(path):
    body, meta, name, inside = collections.OrderedDict(), {}, None, False
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m:
            name, inside = m.group(1), True
            body[name] = []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):   # the metadata comments follow; what else follows is not the kernel's
            inside = False
        t = line.split(";")[0].strip() if not line.lstrip().startswith(";") else ""
        m = re.match(r"^\s*; (\w+)(?::| =) (\d+)", line)
        if m and m.group(1) in META:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
        if not inside:
            continue
        if not t or t[0] == ".":
            if re.match(r"^\.LBB\d+_\d+:", t):
                body[name].append(re.sub(r"^\.LBB\d+_", ".LBB_", t))
            continue
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)
        t = re.sub(r"_Z\w+", "SYM", t)
        body[name].append(" ".join(t.split()))
    names = list(body)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    out = []
    for n, d in zip(names, dem):
        d = re.sub(r"^void ", "", d.replace("(anonymous namespace)::", ""))
        d = d[:d.rindex("(")] if "(" in d else d   # name + template arguments, without the parameter list
        ops = [l for l in body[n] if not l.endswith(":")]
        sha = hashlib.sha256("\n".join(body[n]).encode()).hexdigest()
        mt = meta.get(n, {})
        out.append({"name": d, "base": re.sub(r"<.*", "", d), "n": len(ops), "sha": sha,
                    "meta": " ".join(f"{k} {mt.get(k)}" for k in META)})
    return out


def row(k):
    return f"{k['name']}: {k['n']} instructions, {k['meta']}, sha256 {k['sha'][:16]}"


def main():
    if len(sys.argv) == 2:
        for k in kernels_of(sys.argv[1]):
            print(row(k))
        return 0
    parent, child = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
    key = lambda k: (k["base"], k["sha"], k["n"], k["meta"])
    left = collections.Counter(key(k) for k in child)
    same = 0
    for k in parent:
        hit = left[key(k)] > 0
        if hit:
            left[key(k)] -= 1
            mate = next(c for c in child if key(c) == key(k) and not c.get("taken"))
            mate["taken"] = True
            same += 1
        print(("same      " if hit else "DIFFERENT ") + row(k))
        print("       -> " + (row(mate) if hit else "(no kernel of this name with this stream and metadata)"))
    for c in child:
        if not c.get("taken"):
            print("CHILD ONLY " + row(c))
    print(f"{sys.argv[2]}: {same} of {len(parent)} kernels unchanged, {len(child)} kernels in the child")
    return 0 if same == len(parent) == len(child) else 1


if __name__ == "__main__":
    sys.exit(main())
