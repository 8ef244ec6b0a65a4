"""Builds boofcv_amd/libboofhip.so (hand-written HIP kernels + the C ABI) for gfx950 with hipcc.

hipcc cross-compiles without a GPU.  Every csrc/*.hip is one object; at most max_jobs() compilers run at once, and the link refuses
undefined symbols.  -ffp-contract=off keeps Java's "no fused multiply-add" arithmetic in every kernel;
fp32 divide/sqrt stay correctly rounded.
"""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libboofhip.so")
LIB_EXPERIMENTS = os.path.join(HERE, "libboofhip_exp.so")   # -DBHIP_EXPERIMENTS: ablation / stamp / tile-variant switches (scripts/ only, never shipped)
ARCH = "gfx950"

FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result"]
# Per-source additions.  describe.hip: k_describe's waves loop over key points, and with the whole kernel body inside a loop the machine-level
# loop-invariant code motion parks every fp64 constant of the atan2 / merge / window code in vector registers across it (192 VGPRs, two waves
# per SIMD instead of four); without that pass the kernel keeps its four waves ("describe: persistent waves").
SOURCE_FLAGS = {"describe.hip": ["-mllvm", "-disable-machine-licm"]}


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip"))) + sorted(glob.glob(os.path.join(CSRC, "*.cpp")))


def common_deps():
    """What every object depends on besides its own source."""
    return glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(HERE, "..", "include", "boofhip.h"), os.path.abspath(__file__)]


def max_jobs():
    """Compilers run at once: 16, fewer where MAX_JOBS or the CPUs this process may use are fewer."""
    n = min(16, len(os.sched_getaffinity(0)))
    if os.environ.get("MAX_JOBS"):
        n = min(n, int(os.environ["MAX_JOBS"]))
    return max(1, n)


def needs_build(lib=LIB):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(d) > t for d in sources() + common_deps())


def build(force=False, verbose=False, experiments=False):
    """experiments=True builds libboofhip_exp.so with the timing-experiment switches compiled in (select it with BHIP_LIB=...);
    the default product library contains none of them (tests/test_cabi_symbols.py).
    Only the objects older than their source or than common_deps() are compiled again, then everything is linked; force=True (and
    with it every BHIP_EXP_DEFS variant) compiles all of them.  The skip trusts modification times alone: an object left half-written by
    a killed compiler, or compiled under another HIPCC or environment into the same directory, is linked as it is -- use force=True then."""
    lib = LIB_EXPERIMENTS if experiments else LIB
    extra = []
    if experiments and os.environ.get("BHIP_EXP_DEFS"):
        # compile-time variants for A/B runs: BHIP_EXP_DEFS="-DBHIP_TAP_AUX=1" BHIP_EXP_TAG=sc0 -> libboofhip_exp_sc0.so
        extra = os.environ["BHIP_EXP_DEFS"].split()
        lib = os.path.join(HERE, "libboofhip_exp_%s.so" % os.environ.get("BHIP_EXP_TAG", "variant"))
        force = True
    if not force and not needs_build(lib):
        return lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    objdir = os.path.join(HERE, ("build_exp_" + os.environ.get("BHIP_EXP_TAG", "variant")) if extra else "build_exp" if experiments else "build")
    os.makedirs(objdir, exist_ok=True)
    cmds = []
    newest = max(os.path.getmtime(d) for d in common_deps())
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        if not force and os.path.exists(obj) and os.path.getmtime(obj) > max(newest, os.path.getmtime(src)):
            continue
        cmd = [hipcc, "--offload-arch=" + ARCH] + FLAGS + (["-DBHIP_EXPERIMENTS"] if experiments else []) + extra + SOURCE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        if src.endswith(".cpp"):
            cmd.insert(1, "-x")
            cmd.insert(2, "hip")
        cmds.append((src, cmd))
    # the instantiation units (a few lines of source, the longest compiles) first, then the largest sources: a long compile never starts last
    cmds.sort(key=lambda sc: (not os.path.basename(sc[0]).startswith("background_gmm_"), -os.path.getsize(sc[0])))

    def compile_one(sc):
        if verbose:
            print(" ".join(sc[1]), file=sys.stderr)
        return subprocess.run(sc[1], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)

    pool = ThreadPoolExecutor(max_jobs())
    try:
        for (src, _), p in zip(cmds, pool.map(compile_one, cmds)):
            if p.returncode != 0:
                raise RuntimeError("hipcc failed on %s:\n%s" % (src, p.stdout.decode(errors="replace")))
            if verbose and p.stdout:
                print(p.stdout.decode(errors="replace"), file=sys.stderr)
    finally:
        pool.shutdown(cancel_futures=True)   # after a failure: start no further compiler
    # -z defs: an instantiation that no unit provides fails the link, not the first call
    cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-Wl,-z,defs", "-o", lib] + objs
    subprocess.check_call(cmd)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, experiments="--experiments" in sys.argv))
