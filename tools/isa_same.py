#!/usr/bin/env python3
"""Compare the gfx950 code of kernels between two device assembly files (hipcc -save-temps or
--cuda-device-only -S): the instruction streams with symbol names and labels normalised, and the
resource figures of the kernel descriptors.

    python tools/isa_same.py OLD.s NEW.s 'score_mfma_kernel<1, false, true, 0, 4>=grm_contract_kernel<1>' ...

Each argument pairs the demangled prefix of a kernel in OLD.s with one in NEW.s.  Exit status 1 on a difference."""
import re
import subprocess
import sys

FIGS = (".sgpr_count", ".vgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".sgpr_spill_count", ".vgpr_spill_count")


def kernels(path):
    """mangled name -> (instruction lines, metadata figures)"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if not name.startswith("_Z"):
            continue
        ins = []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith(".") or ln.endswith(":"):
                continue
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", ln.replace(name, "KERNEL")))
        out[name] = [ins, {}]
    # amdhsa.kernels metadata: one YAML item per kernel
    for item in re.split(r"^  - ", text[text.find("amdhsa.kernels"):], flags=re.M)[1:]:
        nm = re.search(r"^\s+\.name:\s+(\S+)", item, re.M)
        if nm and nm.group(1) in out:
            for f in FIGS:
                v = re.search(r"^\s*%s:\s+(\S+)" % re.escape(f), item, re.M)
                if v:
                    out[nm.group(1)][1][f] = v.group(1)
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(res.stdout.split("\n"), names))


def pick(ks, prefix):
    dm = demangle(list(ks))
    hits = [m for d, m in dm.items() if d.replace("void ", "").startswith(prefix)]
    if len(hits) != 1:
        raise SystemExit("%r matches %d kernels" % (prefix, len(hits)))
    return ks[hits[0]]


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for pair in sys.argv[3:]:
        a, b = pair.split("=")
        (ia, fa), (ib, fb) = pick(old, a), pick(new, b)
        count = lambda ins, pre: sum(1 for x in ins if x.startswith(pre))
        same = ia == ib and fa == fb
        bad += not same
        print("%s = %s: %s  (%d instructions, %d MFMA, %d global/buffer loads; %s)" % (
            a, b, "identical" if same else "DIFFERENT", len(ib), count(ib, "v_mfma"),
            count(ib, "global_load") + count(ib, "buffer_load"), " ".join("%s=%s" % (k[1:], v) for k, v in fb.items())))
        if not same:
            ops = lambda ins: sorted(x.split()[0] for x in ins)
            diff = [i for i, (x, y) in enumerate(zip(ia, ib)) if x != y]
            print("  old: %d instructions, figures %s, opcode multiset %s, lines that differ: %d within [%s, %s]" % (
                len(ia), "equal" if fa == fb else fa, "equal" if ops(ia) == ops(ib) else "DIFFERENT", len(diff),
                diff[0] if diff else "-", diff[-1] if diff else "-"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
