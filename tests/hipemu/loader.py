"""TEST INFRASTRUCTURE: builds and opens libmds_emu.so, the host simulator build of csrc/*.hip
(see hipemu.h).  Only the test-suite uses this; the product loader (mds.cabi.load) cannot."""
import collections
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "ball-action-spotting_amd", "csrc")
_LIB = None


def load_emulator():
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-j8", "emu"], cwd=CSRC, check=True)
        from mds.cabi import Lib
        _LIB = Lib(os.path.join(HERE, "libmds_emu.so"))
    return _LIB


Launch = collections.namedtuple("Launch", "kernel gx gy gz bx inst")


def launches():
    """the simulator's launch record since the last reset_launches(): [Launch(kernel expression, grid.x, grid.y, grid.z, block.x,
    inst)]; inst is the kernel instantiation with its template values, spelled as `nm -C` prints the compiled symbol
    ('conv_wgrad_kernel<float, 0, 2, 4, 9>' for the expression 'conv_wgrad_kernel<T, PRO, CI, CO, XL_>')"""
    dll = load_emulator().dll
    dll.hipemu_launch_get.restype = ctypes.c_char_p
    dll.hipemu_launch_get.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint)]
    dll.hipemu_launch_inst.restype = ctypes.c_char_p
    out, dims = [], (ctypes.c_uint * 4)()
    for i in range(dll.hipemu_launch_count()):
        out.append(Launch(dll.hipemu_launch_get(i, dims).decode(), *dims, dll.hipemu_launch_inst(i).decode()))
    return out


def reset_launches():
    load_emulator().dll.hipemu_launch_reset()


def inst_begin():
    """start a window of launched instantiations (inst_seen); independent of launches() / reset_launches() and of the record's cap"""
    load_emulator().dll.hipemu_inst_begin()


def inst_seen():
    """the instantiations launched since inst_begin(), each once"""
    dll = load_emulator().dll
    dll.hipemu_inst_get.restype = ctypes.c_char_p
    return [dll.hipemu_inst_get(i).decode() for i in range(dll.hipemu_inst_count())]
