"""Every kernel instantiation the gfx950 library compiles is launched by a kernel test: on guarded buffers, through Backend.call,
next to a reference (tools/kernel_census.py: the compiled list from the hipcc objects, the launched set from the simulator's record
of instantiations).  No exemption list: a new template value needs a case (tests/test_k_instantiations.py) or has no launch that
reaches it and goes.

The file sorts after every kernel test file on purpose.  In a full `pytest -m "not gpu"` the kernel tests have filled
backends.KERNEL_TEST_INSTANTIATIONS in this very process by the time this test runs, and nothing is run twice; a kernel test file
that did not run here in full before this test (this file on its own, -k, a node id, another order) is run in ONE child pytest
process, which must exit 0 - the verdict is the same.  CPU only: the simulator makes the record."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_census  # noqa: E402


def ran_here_in_full(request):
    """kernel test files whose every CPU test ran in this process before this one: only a run that selects whole files (no -k,
    no node ids, no --deselect, no --lf / --ff / --nf / --sw, at most the `not gpu` marker expression) can say so; any other run
    hands every file to the child process, which can cost time and never a wrong verdict"""
    opt = request.config.option
    partial = [getattr(opt, name, None) for name in ("deselect", "lf", "failedfirst", "newfirst", "stepwise", "stepwise_skip")]
    whole = not opt.keyword and opt.markexpr in ("", "not gpu") and not any(partial) and not any("::" in a for a in request.config.args)
    if not whole:
        return set()
    before = request.session.items[:request.session.items.index(request.node)]
    return {os.path.basename(str(it.fspath)) for it in before}


def test_every_compiled_kernel_instantiation_is_launched_by_a_kernel_test(request):
    import backends
    files = kernel_census.kernel_test_files()
    here = ran_here_in_full(request)
    launched = set(backends.KERNEL_TEST_INSTANTIATIONS)
    launched |= kernel_census.launched_by([f for f in files if f not in here])
    objects = kernel_census.compiled()
    every = {i for insts in objects.values() for i in insts}
    assert len(every) > 500, f"only {len(every)} kernels under csrc/build: the objects are not the library's"
    stray = sorted(launched - every)
    assert not stray, f"{len(stray)} launched names are no compiled instantiation (the simulator and nm spell them differently):\n  " + "\n  ".join(stray)
    missing = kernel_census.missing(objects, launched)
    assert not missing, (f"{len(missing)} of {len(every)} compiled kernel instantiations are launched by no kernel test "
                         f"(add a case to tests/test_k_instantiations.py, or remove the dispatch line that nothing reaches):\n  " + "\n  ".join(missing))
