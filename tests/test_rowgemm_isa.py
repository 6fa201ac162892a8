"""CPU: the hand-managed register double buffer of the W-direct row-owning GEMM survives code generation.

rowgemm_wd_kernel (jyutvoice_amd/csrc/rowgemm_kernel.h) loads its weight fragments by inline asm and waits for them with a
counted s_waitcnt the compiler knows nothing about; tools/check_rowgemm_isa.py compiles the kernels for gfx950 and asserts
that no instruction but those loads and the MFMAs touches the buffer's registers once a load into them has been issued
(a register-allocator copy there would read a register whose load is still in flight).

The same compile yields every kernel's footprint (registers, scratch): compared against profiles/row_kernels_resources.json,
so that a change to the shared row tail (row_tail.h) cannot quietly cost a kernel registers or push it into scratch."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def isa_run(tmp_path_factory):
    """one run of the tool for both tests: (completed process, {kernel: footprint})"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang in this environment")
    table = tmp_path_factory.mktemp("isa") / "resources.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_rowgemm_isa.py"), f"--resources={table}"],
                       capture_output=True, text=True, timeout=900)
    return r, (json.loads(table.read_text()) if table.exists() else None)


def test_register_double_buffer_is_untouched_between_load_and_use(isa_run):
    r, _ = isa_run
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 violations" in r.stdout


def test_row_kernel_footprints_do_not_grow(isa_run):
    """the kernels of rowgemm.hip, rowblock.hip and hiftconv.hip are the recorded ones, and none needs more VGPRs, a larger AGPR
    extent or more scratch than recorded (the rowblock_kernel instantiations at RT = 5 are recorded WITH their 8 - 96 bytes)"""
    r, now = isa_run
    assert now is not None, r.stdout[-3000:] + r.stderr[-2000:]
    with open(os.path.join(REPO, "profiles", "row_kernels_resources.json")) as f:
        recorded = json.load(f)
    assert set(now) == set(recorded), sorted(set(now) ^ set(recorded))
    agprs = lambda k: max(0, k["vgpr"] - k["accum_offset"])      # next free VGPR counts the AGPRs, which begin at accum_offset
    grown = [(name, recorded[name], k) for name, k in sorted(now.items())
             if min(k["vgpr"], k["accum_offset"]) > min(recorded[name]["vgpr"], recorded[name]["accum_offset"])
             or agprs(k) > agprs(recorded[name]) or k["scratch"] > recorded[name]["scratch"]]
    assert not grown, grown
