"""What the compiler reports for the skip-table query kernel (csrc/query_table.hip, pifu_query_tabws_kernel):
no private memory, no spilled vector registers, at most 128 vector registers, and no LDS beyond what the launcher
asks for.  The source is compiled for gfx950 with the flags of monoport_amd/build.py plus the compiler's
kernel-resource-usage remarks; the test reads that report (not the assembly).  Needs hipcc, no GPU.

Why it matters: the kernel's producer waves share their SIMD's vector-memory path with the consumers' weight
stream, and a reload from private memory in front of a job's table loads waits for every load in flight."""
import os
import re
import subprocess
import tempfile

import pytest

from monoport_amd import build as mp_build

SRC = os.path.join(mp_build.CSRC, "query_table.hip")
FIELDS = {
    "vgprs": r"VGPRs: (\d+)",
    "agprs": r"AGPRs: (\d+)",
    "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
    "vgpr_spill": r"VGPRs Spill: (\d+)",
    "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)",
    "lds": r"LDS Size \[bytes/block\]: (\d+)",
}


@pytest.fixture(scope="module")
def report():
    """{kernel symbol: {field: int}} from one device-only compilation of query_table.hip."""
    try:
        hipcc = mp_build._hipcc()
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([hipcc] + mp_build.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                           "-c", SRC, "-o", os.path.join(tmp, "query_table.o")],
                               capture_output=True, text=True)
    except (RuntimeError, OSError) as e:
        pytest.fail("hipcc is needed for this test: %s" % e)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for key, pat in FIELDS.items():
            m = re.search(r"remark:\s+" + pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return kernels


@pytest.mark.parametrize("cout", [1, 3])
def test_tabws_kernel_has_no_private_memory(report, cout):
    names = [k for k in report if "pifu_query_tabws_kernelILi%dEE" % cout in k]
    assert len(names) == 1, sorted(report)
    res = report[names[0]]
    print(names[0], res)
    assert set(res) == set(FIELDS), res
    assert res["scratch"] == 0      # private_segment_fixed_size: not one byte per lane
    assert res["vgpr_spill"] == 0
    assert res["vgprs"] + res["agprs"] <= 128  # four waves per SIMD: both workgroups of a CU resident
    assert res["occupancy"] >= 4
    # all of the kernel's LDS is the dynamic allocation of the launch (kWsLds, held to two workgroups per CU by the
    # static_asserts next to it): the kernel itself declares none on top of what the launcher requests
    assert res["lds"] == 0
