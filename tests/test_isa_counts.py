"""tools/isa_counts.py on a hand-written listing: the classes, the barrier segments, the innermost loop and the metadata line."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTING = """
	.text
toy_kernel:                             ; @toy_kernel
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_lshlrev_b32_e32 v1, 2, v0
	global_load_dwordx4 v[2:5], v1, s[0:1]
	v_cvt_f32_i32_e32 v6, v0
	ds_write_b64 v1, v[2:3]
	s_waitcnt lgkmcnt(0)
	s_barrier
.LBB0_1:                                ; =>This Loop Header: Depth=1
	v_mov_b32_e32 v7, 0
.LBB0_2:                                ;   This Inner Loop Header: Depth=2
	ds_read_b64 v[8:9], v1
	ds_read_b64 v[10:11], v1 offset:8
	v_pk_fma_f32 v[12:13], v[8:9], v[10:11], v[12:13]
	v_exp_f32_e32 v14, v12
	v_add_f32_e32 v15, v14, v13
	v_add_u32_e32 v1, 0x150, v1
	s_add_i32 s2, s2, -1
	s_cmp_eq_u32 s2, 0
	s_cbranch_scc0 .LBB0_2
; %bb.3:
	v_mfma_f32_16x16x16_bf16 v[16:19], v[8:9], v[10:11], v[16:19]
	s_cbranch_vccnz .LBB0_1
; %bb.4:
	s_endpgm
.Lfunc_end0:
	.size	toy_kernel, .Lfunc_end0-toy_kernel
	.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .name:           toy_kernel
    .private_segment_fixed_size: 12
    .sgpr_spill_count: 1
    .vgpr_count:     20
    .vgpr_spill_count: 2
...
	.end_amdgpu_metadata
"""


def test_isa_counts(tmp_path):
    src = tmp_path / "toy.s"
    src.write_text(LISTING)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_counts.py"), str(src), "toy_"], capture_output=True, text=True, check=True).stdout
    assert "vgprs 20  agprs 0  scratch bytes 12  vgpr spills 2  sgpr spills 1" in out
    rows = {}
    for ln in out.splitlines():
        f = ln.split()
        if f[:1] == ["mfma"]:
            assert f == ["mfma", "pk32", "fp32", "cvt", "trans", "int", "valu", "ldsr", "ldsw", "gld"]
        elif f[:1] == ["segment"] or f[:1] == [".LBB0_2"]:
            rows[" ".join(f[:-10])] = [int(x) for x in f[-10:]]
    #                                  mfma pk32 fp32 cvt trans int valu ldsr ldsw gld
    assert rows == {"segment 0":      [0, 0, 0, 1, 0, 1, 2, 0, 1, 1],
                    "segment 1":      [1, 1, 1, 0, 1, 2, 6, 2, 0, 0],
                    ".LBB0_2 s1 n9":  [0, 1, 1, 0, 1, 1, 4, 2, 0, 0]}       # the inner loop only: the outer one holds it
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_counts.py"), str(src), "no_such_kernel"], capture_output=True, text=True)
    assert bad.returncode != 0
