"""Static instruction mix per kernel of a gfx950 assembly listing (hipcc -S --cuda-device-only with the flags of build.py).

    python tools/isa_mix.py <file.s> [kernel name filter (regex on the demangled name)]

Per kernel: instructions before the first MFMA, between the first and the last MFMA, and after the last one, by class (MFMA, other
vector ALU, LDS, vector memory, scalar ALU / memory, branches, s_waitcnt, s_barrier), plus VGPRs, scratch bytes, occupancy and code size."""
import collections
import re
import subprocess
import sys


def klass(op):
    if "mfma" in op:
        return "mfma"
    if op.startswith("s_cbranch") or op.startswith("s_branch"):
        return "branch"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "scalar"
    return "other"


def main():
    path = sys.argv[1]
    filt = re.compile(sys.argv[2] if len(sys.argv) > 2 else ".")
    kernels, meta, name = collections.OrderedDict(), {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m:
            name = m.group(1)
            kernels[name] = []
            continue
        if name is None:
            continue
        t = line.strip()
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy|codeLenInByte|LDSByteSize)(?::| =) (\d+)", t)
        if m:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
            continue
        if not t or t[0] in ".;" or t.endswith(":"):
            continue
        kernels[name].append(t.split()[0])
    names = list(kernels)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    cols = ["mfma", "valu", "lds", "vmem", "scalar", "branch", "waitcnt", "barrier"]
    for n, d in zip(names, dem):
        d = re.sub(r"\(anonymous namespace\)::", "", d)
        d = re.sub(r"^void ", "", re.sub(r"\(.*", "", d))
        ops = kernels[n]
        if not filt.search(d) or not any("mfma" in o for o in ops):
            continue
        idx = [i for i, o in enumerate(ops) if "mfma" in o]
        parts = {"before": ops[:idx[0]], "mfma section": ops[idx[0]:idx[-1] + 1], "after": ops[idx[-1] + 1:]}
        mt = meta.get(n, {})
        print(f"{d}: vgpr {mt.get('NumVgprs')} scratch {mt.get('ScratchSize')} occupancy {mt.get('Occupancy')} code {mt.get('codeLenInByte')} B")
        for pn, po in parts.items():
            c = collections.Counter(klass(o) for o in po)
            extra = collections.Counter(o for o in po if o in ("v_ldexp_f32", "ds_write_b32", "ds_write2_b32", "ds_read_u8", "ds_read_b128"))
            print(f"   {pn:13s} total {len(po):5d}  " + "  ".join(f"{k} {c.get(k, 0)}" for k in cols)
                  + ("   (" + ", ".join(f"{k} {v}" for k, v in sorted(extra.items())) + ")" if extra else ""))


if __name__ == "__main__":
    main()
