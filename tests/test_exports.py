"""CPU-side check of the export surface: nothing of the host files' shared internals (namespace lcd_internal, csrc/lcd_host_internal.h) is a dynamic symbol."""
import os
import shutil
import subprocess

import pytest


def _nm():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "llvm", "bin", "llvm-nm"), os.path.join(rocm, "lib", "llvm", "bin", "llvm-nm"), shutil.which("nm")):
        if c and os.path.exists(c):
            return c
    return None


def test_internal_namespace_not_exported():
    from longcalld_amd import _lib
    nm = _nm()
    if nm is None:
        pytest.skip("neither llvm-nm in the ROCm tree nor nm on PATH")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-400:]
    names = [ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()]
    assert "lcd_init" in names and len(names) >= 100   # (the tool listed the library's symbols at all)
    leaked = [n for n in names if "lcd_internal" in n]   # mangled names carry the namespace as 12lcd_internal
    assert not leaked, f"internal names exported from liblcd_hotpath.so: {leaked[:10]}"
