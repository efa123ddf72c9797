"""Build libmpengine.so (the HIP kernels + C ABI) in-tree with hipcc for gfx950.

    python -m graphgym_amd.build            # build if sources are newer than the .so
    python -m graphgym_amd.build --force

The .so is git-ignored but travels to the GPU box with the gpurun snapshot.
hipcc cross-compiles without a GPU, so this also runs in the CPU-only container.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(CSRC, "libmpengine.so")
SOURCES = ["spmm.hip", "fused.hip", "fused_hot.hip", "csr_build.hip", "attn.hip", "ego.hip", "edge.hip", "codes.hip", "link.hip", "sample.hip", "neighbor.hip", "collate.hip", "structure.hip", "centrality.hip", "gemm.hip", "dense_x3.hip", "bn.hip", "bn_drop.hip", "util.hip", "probe.hip", "loss.hip", "evalmetrics.hip", "pair.hip"]
HEADERS = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "vecio.h"), os.path.join(CSRC, "bf16x3.h"), os.path.join(CSRC, "fused_pc.h"), os.path.join(CSRC, "draws.h"), os.path.join(CSRC, "act.h"), os.path.join(CSRC, "bn_kernels.h"),
           os.path.join(ROOT, "include", "mp_engine.h"), os.path.join(ROOT, "include", "mp_eval.h"),
           os.path.join(ROOT, "include", "mp_structure.h"), os.path.join(ROOT, "include", "mp_spline.h"),
           os.path.join(ROOT, "include", "mp_neighbor.h"), os.path.join(ROOT, "include", "mp_pair.h"),
           os.path.join(ROOT, "include", "mp_maxbwd.h")]
ARCH = "gfx950"
# per-source flags.  fused_hot.hip (the hot kernels of fused_pc.h alone): uniform branches stay branches, not structurized
# into two one-sided regions — the gather's per-row choice of cache policy otherwise leaves control-flow paths with zero
# or two loads, and the wait counting falls back to vmcnt(0) at every consumed row (see the file)
EXTRA_FLAGS = {"fused_hot.hip": ["-mllvm", "-structurizecfg-skip-uniform-regions=true"]}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    hipcc = _hipcc()
    objs = []
    procs = []
    for s in SOURCES:
        obj = os.path.join(CSRC, s.replace(".hip", ".o"))
        objs.append(obj)
        cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-c",
               os.path.join(CSRC, s), "-o", obj] + EXTRA_FLAGS.get(s, [])
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {s}:\n{out.decode(errors='replace')}")
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
