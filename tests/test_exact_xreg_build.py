"""Guard of the build, on the CPU: the register budget of the exact kernel's cross-wave-GEMM3 (XW) instances, read from
the kernel metadata of the code objects inside the built libpmf_hip.so (extracted the way tests/test_build_scan.py does).

An XW instance runs two waves per SIMD, 256 registers each.  The register-resident-X variants (XR, the last template
argument) add 96 registers to an instance and are built only where that still fits without scratch (pmf_common.h,
pmf_exact_has_xr, the rule the host and pmf_k_fused.hip share): a variant that spills would be slower than the LDS reads it replaces, and
nothing but this test would notice, because the results are bit-identical.

The two instances that store D as bf16 with mixed noise models and batch layers sat at 256 VGPRs with 8 and 32 bytes of
scratch before there was anything to add; they now recompute their GEMM3 and load addresses per tile instead of pinning
them for the launch (pmf_fused.hip.inc, TIGHT) and fit too: 244 and 256 VGPRs, no scratch.
"""
import importlib.util
import re
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "pathmatfac.jl_amd" / "libpmf_hip.so"
# pmf_fused_kernel<KB, NW, RBW, BMODE, MIXED, GM, DB, XW, XR>
SYM = re.compile(r"_Z16pmf_fused_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)ELb([01])ELi(\d)ELb([01])ELb([01])ELb([01])EEv9FusedArgs$")
# the instances DESIGN.md section 4.1 lists as register-resident: (BMODE, MIXED, DB)
RESIDENT = {(0, 0, 0), (0, 0, 1)}


def _scanner():
    spec = importlib.util.spec_from_file_location("scan_agpr", ROOT / "scripts" / "scan_agpr_pair_copy.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _xw_kernels():
    """{(BMODE, MIXED, DB, XR): (vgprs, scratch bytes, symbol)} of every XW instance in the built library."""
    s = _scanner()
    out = {}
    if not LIB.exists():
        return out
    with tempfile.TemporaryDirectory() as td:
        for i, co in enumerate(s.code_objects(LIB)):
            if b"pmf_fused_kernel" not in co:
                continue
            f = Path(td) / f"co{i}.o"
            f.write_bytes(co)
            notes = subprocess.run([str(s.LLVM / "llvm-readelf"), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                m = SYM.match(name)
                if not m:
                    continue
                kb, nw, rbw, bmode, mixed, gm, db, xw, xr = (int(x) for x in m.groups())
                if not xw:
                    continue
                assert (kb, nw, rbw, gm) == (2, 8, 1, 0), name
                out[(bmode, mixed, db, xr)] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)), name)
    return out


KERNELS = _xw_kernels()


def test_library_holds_the_xw_instances():
    assert LIB.exists(), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    # LDS-read instance of every (BMODE, MIXED, DB): the PMF_XREG=0 side of the switch, and what the others run
    assert {k[:3] for k in KERNELS if k[3] == 0} == {(b, m, d) for b in range(3) for m in range(2) for d in range(2)}, sorted(KERNELS)


def test_register_resident_instances_are_the_listed_ones():
    assert {k[:3] for k in KERNELS if k[3] == 1} == RESIDENT, sorted(KERNELS)


@pytest.mark.parametrize("key", sorted(KERNELS) or [None], ids=lambda k: "none" if k is None else "bmode%d-mixed%d-bf16%d-xreg%d" % k)
def test_xw_instance_fits_two_waves_per_simd_without_scratch(key):
    assert key is not None, "no XW kernel found in the built library"
    vgprs, scratch, name = KERNELS[key]
    print(f"{name}: {vgprs} VGPRs, {scratch} B scratch")
    assert vgprs <= 256, (name, vgprs)
    assert scratch == 0, (name, scratch)
