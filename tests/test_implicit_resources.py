"""The register budget of the implicit stepper's kernels (csrc/saa_opimp.hip), from a cross-compile: no scratch and no spill in
any kernel - they are node and vector passes, bound by memory, so each keeps the full eight waves per SIMD - and the rows as
hipcc gives them, pinned as tests/test_tangent_resources.py pins its rows."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/kernel_resources.py --file=saa_opimp.hip: sgpr vgpr sgpr_spill vgpr_spill scratch occupancy
OPIMP_ROWS = {
    "saa::opimp_mass_check_kernel": (18, 6, 0, 0, 0, 8),
    "saa::opimp_setup_kernel": (28, 18, 0, 0, 0, 8),
    "saa::opimp_dot_final_kernel": (15, 9, 0, 0, 0, 8),
    "saa::opimp_accel_kernel": (44, 30, 0, 0, 0, 8),
    "saa::opimp_mask_kernel": (26, 8, 0, 0, 0, 8),
    "saa::opimp_predict_kernel": (26, 12, 0, 0, 0, 8),
    "saa::opimp_residual_kernel": (62, 54, 0, 0, 0, 8),
    "saa::opimp_newton_final_kernel": (17, 40, 0, 0, 0, 8),
    "saa::opimp_cg_update_kernel": (36, 38, 0, 0, 0, 8),
    "saa::opimp_cg_direction_kernel": (34, 30, 0, 0, 0, 8),
    "saa::opimp_newton_update_kernel": (24, 12, 0, 0, 0, 8),
    "saa::opimp_finish_kernel": (38, 22, 0, 0, 0, 8),
    "void saa::opimp_shifted_node_kernel<true, true>": (38, 26, 0, 0, 0, 8),
    "void saa::opimp_shifted_node_kernel<true, false>": (32, 29, 0, 0, 0, 8),
    "void saa::opimp_shifted_node_kernel<false, true>": (36, 26, 0, 0, 0, 8),
    "void saa::opimp_shifted_node_kernel<false, false>": (28, 22, 0, 0, 0, 8),
}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_implicit_kernels_use_no_scratch_and_keep_eight_waves():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_opimp.hip"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    print(out.stdout)
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = tuple(int(v) for v in f[-6:])
    assert set(rows) == set(OPIMP_ROWS)
    for name, (sgpr, vgpr, sspill, vspill, scratch, occ) in rows.items():
        assert sspill == 0 and vspill == 0 and scratch == 0 and occ == 8, (name, rows[name])
    assert rows == OPIMP_ROWS
