"""The register budget of the finite-strain stress passes (csrc/saa_stress_fs.hip), from a cross-compile: no scratch and no
spill in any instantiation, the order-2 passes at no more than 256 vector registers - two waves per SIMD, the occupancy of the
force pass whose geometry table they read -, and the rows as hipcc gives them, pinned as tests/test_tangent_resources.py pins
its own.  Template arguments: material (1 svk, 2 neo-Hooke), measure (0 PK2, 1 Cauchy)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/kernel_resources.py --file=saa_stress_fs.hip: sgpr vgpr sgpr_spill vgpr_spill scratch occupancy
STRESS_FS_ROWS = {
    "void saa::stress_fs_p2_kernel<1, 0>": (87, 204, 0, 0, 0, 2),
    "void saa::stress_fs_p1_kernel<1, 0>": (56, 98, 0, 0, 0, 4),
    "void saa::stress_fs_p2_kernel<1, 1>": (93, 242, 0, 0, 0, 2),
    "void saa::stress_fs_p1_kernel<1, 1>": (62, 138, 0, 0, 0, 3),
    "void saa::stress_fs_p2_kernel<2, 0>": (106, 252, 0, 0, 0, 2),
    "void saa::stress_fs_p1_kernel<2, 0>": (76, 153, 0, 0, 0, 3),
    "void saa::stress_fs_p2_kernel<2, 1>": (106, 252, 0, 0, 0, 2),
    "void saa::stress_fs_p1_kernel<2, 1>": (76, 149, 0, 0, 0, 3),
}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_finite_strain_stress_kernels_use_no_scratch_and_keep_two_waves():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_stress_fs.hip"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    print(out.stdout)
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = tuple(int(v) for v in f[-6:])
    assert set(rows) == set(STRESS_FS_ROWS)
    for name, (sgpr, vgpr, sspill, vspill, scratch, occ) in rows.items():
        assert sspill == 0 and vspill == 0 and scratch == 0, (name, rows[name])
        if "stress_fs_p2_kernel" in name:
            assert vgpr <= 256 and occ >= 2, (name, rows[name])
    assert rows == STRESS_FS_ROWS
