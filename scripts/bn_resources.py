"""Compiled shape of the BatchNorm kernels (csrc/bn.hip, csrc/bn_drop.hip) for gfx950, without a device: VGPRs, scratch,
LDS and waves per SIMD of every instantiation from hipcc's -Rpass-analysis=kernel-resource-usage, as a markdown table.

    python scripts/bn_resources.py                  # this tree
    python scripts/bn_resources.py --against DIR    # and, per kernel, the kernels of the tree at DIR that it replaces:
                                                    # exit status 1 if one has scratch, another LDS size or fewer waves

DIR holds the commit before the three kernel families were folded into bn_kernels.h; replaces() below maps names."""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
FIELDS = {"VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "waves",
          "LDS Size [bytes/block]": "lds"}


def resources(root):
    """{demangled kernel name without arguments: {vgpr, scratch, waves, lds}} of the two sources under root"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        procs = [subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", s + ".hip", "-o",
                                   os.path.join(tmp, s + ".o"), "-Rpass-analysis=kernel-resource-usage"],
                                  cwd=os.path.join(root, "graphgym_amd", "csrc"), stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT, text=True) for s in ("bn", "bn_drop")]
        logs = [p.communicate()[0] for p in procs]
        if any(p.returncode for p in procs):
            raise RuntimeError("\n".join(logs))
    cur = None
    for line in "\n".join(logs).splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run([CXXFILT, m.group(2)], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"^void ", "", name)
            name = name[:name.index(">(") + 1] if ">(" in name else name[:name.index("(")]
            cur = out.setdefault(name.replace("mp::", ""), {})
        elif m.group(1) in FIELDS and cur is not None:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def replaces(name):
    """the kernels of the tree before the merge whose work the kernel `name` does"""
    m = re.match(r"(\w+)<(.*)>$", name)
    if not m:
        return [name]
    k, a = m.group(1), [v.strip() for v in m.group(2).split(",")]
    if k == "bn_fwd_stats_kernel":
        return [f"bn_colsum_kernel<{a[0]}, 0>"]
    if k == "bn_bwd_finalize_kernel":
        return ["bn_drop_bwd_finalize_kernel" if a[0] == "double" else "bn_bwd_finalize_kernel"]
    if k == "bn_apply_fwd_kernel":
        ws, wx, form, act, drop = a[0], a[1], int(a[2]), int(a[3]), a[4] == "true"
        if drop:
            return [f"bn_drop_apply_kernel<{ws}, {wx}, {form}, {act}>"]
        cat = "true" if form == 2 else "false"
        if act <= 1:
            return [f"bn_apply_kernel<{wx}, 0>"] if form == 0 else [f"bn_apply_skip_kernel<{ws}, {wx}, {cat}>"]
        return [f"bn_apply_act_kernel<{wx}, {act}>"] if form == 0 else [f"bn_apply_skip_act_kernel<{ws}, {wx}, {cat}, {act}>"]
    if k in ("bn_bwd_stats_kernel", "bn_bwd_apply_kernel"):
        w, act, zsrc, drop = a[0], int(a[1]), int(a[2]), a[3] == "true"      # zsrc: 0 x alone, 1 x (+ skip), 2 y
        stats = k == "bn_bwd_stats_kernel"
        if drop:
            if stats:
                return [f"bn_drop_colsum_kernel<{w}, {act}>"]
            return [f"bn_drop_apply_bwd_g_kernel<{w}>"] if zsrc == 0 else [f"bn_drop_apply_bwd_kernel<{w}, {act}>"]
        old = []
        if zsrc != 1:      # the kernels with the run-time relu flag / the mask from y
            old += [f"bn_colsum_kernel<{w}, 1>"] + ([f"bn_colsum_kernel<{w}, 2>"] if zsrc == 2 else []) if stats else [f"bn_apply_kernel<{w}, 1>"]
        if act >= 1 and zsrc != 2:
            old.append(f"{'bn_colsum_act_kernel' if stats else 'bn_apply_bwd_act_kernel'}<{w}, {act}>")
        return old
    return [name]


def main():
    new = resources(ROOT)
    old = resources(sys.argv[sys.argv.index("--against") + 1]) if "--against" in sys.argv else None
    bad = 0
    print("| kernel | VGPRs | scratch B | LDS B | waves/SIMD |" + (" replaces (VGPRs, LDS B, waves/SIMD) |" if old else ""))
    print("|---|---|---|---|---|" + ("---|" if old else ""))
    for name in sorted(new):
        r = new[name]
        row = f"| `{name}` | {r['vgpr']} | {r['scratch']} | {r['lds']} | {r['waves']} |"
        if old is not None:
            cells = []
            for o in replaces(name):
                if o not in old:
                    cells.append(f"`{o}`: not in DIR")
                    bad += not (name == o or "<" not in name)
                    continue
                q = old[o]
                ok = r["scratch"] == 0 and r["lds"] == q["lds"] and r["waves"] >= q["waves"]
                bad += not ok
                cells.append(f"`{o}` ({q['vgpr']}, {q['lds']}, {q['waves']})" + ("" if ok else " **WORSE**"))
            row += " " + "; ".join(cells) + " |"
        print(row)
    if old is not None:
        print(f"\n{len(new)} kernels, {bad} worse than what they replace")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
