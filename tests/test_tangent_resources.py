"""The register budget of the tangent element passes (csrc/saa_optan.hip), from a cross-compile: no scratch and no spill in
any instantiation, the order-2 passes at no more than 256 vector registers - two waves per SIMD, the occupancy of the force pass
they sit next to -, and the rows as hipcc gives them, pinned as tests/test_kernel_resources.py pins its rows."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/kernel_resources.py --file=saa_optan.hip: sgpr vgpr sgpr_spill vgpr_spill scratch occupancy
OPTAN_ROWS = {
    "void saa::optan_elem_p2_kernel<1>": (38, 254, 0, 0, 0, 2),
    "void saa::optan_elem_p1_kernel<1>": (22, 110, 0, 0, 0, 4),
    "void saa::optan_elem_p2_kernel<2>": (106, 242, 0, 0, 0, 2),
    "void saa::optan_elem_p1_kernel<2>": (18, 126, 0, 0, 0, 4),
}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_tangent_kernels_use_no_scratch_and_keep_two_waves():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_optan.hip"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    print(out.stdout)
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = tuple(int(v) for v in f[-6:])
    assert set(rows) == set(OPTAN_ROWS)
    for name, (sgpr, vgpr, sspill, vspill, scratch, occ) in rows.items():
        assert sspill == 0 and vspill == 0 and scratch == 0, (name, rows[name])
        if "optan_elem_p2_kernel" in name:
            assert vgpr <= 256 and occ >= 2, (name, rows[name])
    assert rows == OPTAN_ROWS
