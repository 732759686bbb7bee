"""The register budget of the kernels that follow the time step (csrc/saa_opdt.hip), from a cross-compile: no scratch and no
spill in any instantiation, the bound passes at two waves per SIMD or more - the 45 doubles of the 9x9 triangle next to the point
law -, and the rows as hipcc gives them, pinned as tests/test_tangent_resources.py pins its rows."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/kernel_resources.py --file=saa_opdt.hip: sgpr vgpr sgpr_spill vgpr_spill scratch occupancy
OPDT_ROWS = {
    "saa::opdt_bound_final_kernel": (29, 19, 0, 0, 0, 8),
    "saa::opdt_set_dt_kernel": (24, 46, 0, 0, 0, 8),
    "void saa::opdt_bound_p2_kernel<2>": (70, 198, 0, 0, 0, 2),
    "void saa::opdt_bound_p1_kernel<2>": (46, 164, 0, 0, 0, 3),
    "void saa::opdt_bound_p2_kernel<1>": (56, 186, 0, 0, 0, 2),
    "void saa::opdt_bound_p1_kernel<1>": (42, 160, 0, 0, 0, 3),
}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_dt_follow_kernels_use_no_scratch_and_keep_two_waves():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_opdt.hip"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    print(out.stdout)
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = tuple(int(v) for v in f[-6:])
    assert set(rows) == set(OPDT_ROWS)
    for name, (sgpr, vgpr, sspill, vspill, scratch, occ) in rows.items():
        assert sspill == 0 and vspill == 0 and scratch == 0, (name, rows[name])
        assert vgpr <= 256 and occ >= 2, (name, rows[name])
    assert rows == OPDT_ROWS
