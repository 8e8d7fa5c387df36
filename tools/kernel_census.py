"""Developer tool and test helper (no GPU needed): which compiled kernel instantiations does a kernel test launch?

    python tools/kernel_census.py            # table per family and per object; exit 1 if an instantiation was never launched
    python tools/kernel_census.py -v         # ... and the name of every unlaunched instantiation

compiled: the `__device_stub__` symbols of the hipcc objects (csrc/build/k_*.o, rebuilt by make when stale), demangled by nm -C:
'conv_wgrad_kernel<float, 0, 2, 4, 9>'.  launched: the set tests/backends.py keeps (KERNEL_TEST_INSTANTIATIONS) - what a successful
Backend.call() / Backend.rc() launched on the simulator, i.e. on guarded buffers from a kernel test; the simulator spells an
instantiation exactly as nm does (tests/hipemu/hipemu.h, inst_name).  The kernel tests run in ONE child pytest process
(`-m "not gpu"`), which must exit 0.  tests/test_zz_kernel_census.py is the same comparison inside the suite."""
import collections
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ball-action-spotting_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")

# the files whose tests launch single kernels on guarded buffers through Backend.call (module, predictor and train-ops tests launch
# through plans: a whole-model comparison does not pin one variant, and Backend.call never sees those launches anyway)
KERNEL_TEST_GLOBS = ["test_k_*.py", "test_launch_geometry.py", "test_guard_bands.py", "test_arena_placement.py", "test_golden_hip.py",
                     "test_deterministic_kernels.py", "test_device_rng_kernel.py", "test_eval_*.py", "test_mixup.py", "test_metrics.py",
                     "test_spotting.py", "test_frames.py", "test_frames_ingest.py"]


def kernel_test_files():
    """base names of the kernel-level test files, sorted"""
    return sorted({os.path.basename(p) for g in KERNEL_TEST_GLOBS for p in glob.glob(os.path.join(TESTS, g))})


def _nm():
    for c in (shutil.which("nm"), "/opt/rocm/lib/llvm/bin/llvm-nm", shutil.which("llvm-nm")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no nm / llvm-nm found")


def instantiation(symbol):
    """'void __device_stub__conv_wgrad_kernel<float, 0, 2, 4, 9>(mds_conv_wgrad_args, int, ...)' -> 'conv_wgrad_kernel<float, 0, 2, 4, 9>':
    the name up to the argument list - the first '(' outside template brackets"""
    s = symbol.split("__device_stub__", 1)[1]
    depth = 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return s[:i]
    return s


def compiled(build=True):
    """{object name: sorted instantiations} of the gfx950 library's objects; make brings stale objects up to date first"""
    if build:
        subprocess.run(["make", "-s", "-j8", "all"], cwd=CSRC, check=True)
    out = {}
    for obj in sorted(glob.glob(os.path.join(CSRC, "build", "k_*.o"))):
        if obj.endswith(".emu.o") or not re.fullmatch(r"k_[a-z0-9]+\.o", os.path.basename(obj)):
            continue
        text = subprocess.run([_nm(), "-C", obj], capture_output=True, text=True, check=True).stdout
        out[os.path.basename(obj)] = sorted({instantiation(l) for l in text.splitlines() if "__device_stub__" in l})
    assert out, f"no objects under {CSRC}/build"
    return out


def launched_by(files):
    """the instantiations the kernel tests of `files` (base names under tests/) launch: one child pytest process, `-m "not gpu"`;
    raises when it does not exit 0"""
    if not files:
        return set()
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "launched.json")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dump] + [os.path.join(TESTS, f) for f in files],
                           cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0 or not os.path.exists(dump):
            raise RuntimeError(f"the kernel tests' child process exited {r.returncode}:\n{r.stdout[-4000:]}\n{r.stderr[-2000:]}")
        with open(dump) as f:
            return set(json.load(f))


def _child(dump, files):
    """pytest in this process, so that backends.KERNEL_TEST_INSTANTIATIONS is the module the tests filled"""
    import pytest
    rc = int(pytest.main(["-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider"] + files))
    if rc == 0:
        import backends
        with open(dump, "w") as f:
            json.dump(sorted(backends.KERNEL_TEST_INSTANTIATIONS), f)
    return rc


def family(inst):
    return inst.split("<", 1)[0]


def table(objects, launched):
    """text: per family and per object, compiled and never launched"""
    rows = ["| family | compiled | never launched by a kernel test |", "|---|---|---|"]
    fam = collections.OrderedDict()
    for insts in objects.values():
        for i in insts:
            fam.setdefault(family(i), set()).add(i)
    for name, insts in sorted(fam.items(), key=lambda kv: (-len(kv[1] - launched), -len(kv[1]), kv[0])):
        rows.append(f"| `{name}` | {len(insts)} | {len(insts - launched)} |")
    rows += ["", "| object | compiled | never launched by a kernel test |", "|---|---|---|"]
    for obj, insts in objects.items():
        rows.append(f"| `{obj}` | {len(insts)} | {len(set(insts) - launched)} |")
    every = {i for insts in objects.values() for i in insts}
    rows.append(f"| all (distinct) | {len(every)} | {len(every - launched)} |")
    return "\n".join(rows)


def missing(objects, launched):
    return sorted({i for insts in objects.values() for i in insts} - launched)


def main(argv):
    if argv[:1] == ["--child"]:
        return _child(argv[1], argv[2:])
    objects = compiled()
    launched = launched_by(kernel_test_files())
    every = {i for insts in objects.values() for i in insts}
    print(table(objects, launched))
    stray = sorted(launched - every)
    if stray:
        print(f"\n{len(stray)} launched names are no compiled instantiation (the simulator and nm disagree on their spelling):\n  " + "\n  ".join(stray))
    miss = missing(objects, launched)
    if "-v" in argv and miss:
        print(f"\n{len(miss)} never launched:\n  " + "\n  ".join(miss))
    print(f"\n{len(every)} instantiations compiled, {len(miss)} never launched by a kernel test")
    return 1 if (miss or stray) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
