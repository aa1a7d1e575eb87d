"""The C-ABI boundary of the one-launch SGD step (csrc/sgd.hip), without a GPU: the item struct against the table fused_sgd.py writes
from numpy, the argument checks that return before any launch, and the kernel id's name."""
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_item_struct_matches_the_numpy_table():
    from vm_asr_amd import fused_sgd
    fields = ("p", "g", "buf", "lp", "lpt", "n", "weight_decay", "vec", "rows", "cols")
    names = ("p", "g", "buf", "lp", "lpt", "n", "wd", "vec", "rows", "cols")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vmasr_hip.h"\nint main(void){ printf("%zu", sizeof(vmasr_sgd_item));\n'
            + "".join(f'printf(" %zu", offsetof(vmasr_sgd_item, {f}));\n' for f in fields) + "return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as fh:
            fh.write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    dt = fused_sgd._ITEM
    assert got == [dt.itemsize] + [dt.fields[n][1] for n in names]
    assert dt.itemsize == 64 and dt.names == names


def test_bad_arguments_are_refused_before_any_launch():
    from vm_asr_amd import _lib
    lib = _lib.lib()
    assert {"vmasr_sgd_step", "vmasr_sgd_step_guarded"} <= set(_lib.SYMBOLS)
    # (addresses that are never dereferenced on the host: the checks return first)
    tab = (ctypes.c_char * 64)()
    a = ctypes.cast(tab, ctypes.c_void_p)
    assert lib.vmasr_sgd_step(None, a, 1, 4, a, 0.9, 1, None) == -1 and b"null" in lib.vmasr_last_error()
    assert lib.vmasr_sgd_step(a, None, 1, 4, a, 0.9, 1, None) == -1
    assert lib.vmasr_sgd_step(a, a, 1, 4, None, 0.9, 1, None) == -1 and b"null" in lib.vmasr_last_error()
    assert lib.vmasr_sgd_step_guarded(a, a, 1, 4, a, 0.9, 1, None, None) == -1 and b"null" in lib.vmasr_last_error()
    for n in (0, -3):
        assert lib.vmasr_sgd_step(a, a, n, 4, a, 0.9, 1, None) == -1 and b"nchunks" in lib.vmasr_last_error()
        assert lib.vmasr_sgd_step_guarded(a, a, n, 4, a, 0.9, 1, a, None) == -1 and b"nchunks" in lib.vmasr_last_error()
    for mu in (1.0, 1.5, -0.1, float("nan")):
        assert lib.vmasr_sgd_step(a, a, 1, 4, a, mu, 0, None) == -1 and b"momentum" in lib.vmasr_last_error()
        assert lib.vmasr_sgd_step_guarded(a, a, 1, 4, a, mu, 0, a, None) == -1 and b"momentum" in lib.vmasr_last_error()


def test_kernel_id_has_a_name():
    from vm_asr_amd import _lib
    names = [_lib.lib().vmasr_prof_name(k) for k in range(_lib.K_COUNT)]
    assert b"sgd" in names and len(set(names)) == _lib.K_COUNT and _lib.lib().vmasr_prof_name(_lib.K_COUNT) == b""
