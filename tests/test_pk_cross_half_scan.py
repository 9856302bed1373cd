"""tools/check_pk_cross_half.py (CPU): no packed f32 instruction whose low result reads a source's high half in any kernel of the built
libraries outside the objects the build lists as known carriers, none at all in the bf16 x 3 attention kernel, and the positive control:
a kernel that holds the form is refused, the same kernel without op_sel is not."""
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = os.path.join(ROOT, "tools", "check_pk_cross_half.py")
CSRC = os.path.join(ROOT, "ipdm-pytorch_amd", "csrc")
KNOWN = ["art.o", "conv_direct.o", "conv_nm.o", "conv_wino2.o", "conv_wino3.o", "conv_ws.o"]      # csrc/Makefile PK_CROSS_KNOWN

SRC = r"""
#include <hip/hip_runtime.h>
typedef float f32x2 __attribute__((ext_vector_type(2)));
__global__ void pk_probe(f32x2 *p)
{
    f32x2 a = p[threadIdx.x], b = p[threadIdx.x + 64], c;
    asm volatile("v_pk_add_f32 %0, %1, %2 OPSEL" : "=v"(c) : "v"(a), "v"(b));
    p[threadIdx.x + 128] = c;
}
"""


def _scan(*args):
    return subprocess.run([sys.executable, SCAN] + list(args), capture_output=True, text=True, timeout=600)


def test_built_libraries_have_no_new_cross_half_packed_op():
    objs = sorted(glob.glob(os.path.join(CSRC, "*.o")))
    assert os.path.join(CSRC, "attn_bx3.o") in objs, "csrc/*.o missing: run __graft_entry__.build()"
    allow = [x for k in KNOWN for x in ("--allow", k)]
    r = _scan(*(allow + objs))
    assert r.returncode == 0 and " 0 cross-half refused" in r.stdout, r.stdout[-2000:]
    r = _scan(os.path.join(CSRC, "attn_bx3.o"))
    assert r.returncode == 0 and " 0 packed f32 instruction(s)" in r.stdout, r.stdout[-2000:]


def test_the_scanner_refuses_the_form(tmp_path):
    def build(opsel, name):
        src, obj = tmp_path / (name + ".hip"), str(tmp_path / (name + ".o"))
        src.write_text(SRC.replace("OPSEL", opsel))
        subprocess.run(["hipcc", "-O3", "--offload-arch=gfx950", "-c", str(src), "-o", obj], check=True, capture_output=True, timeout=600)
        return obj
    bad = _scan(build("op_sel:[0,1] op_sel_hi:[1,0]", "cross"))
    assert bad.returncode == 1 and "PACKED F32 CROSS-HALF" in bad.stdout and "pk_probe" in bad.stdout, bad.stdout[-2000:]
    assert _scan("--allow", "cross2.o", build("op_sel:[0,1] op_sel_hi:[1,0]", "cross2")).returncode == 0
    assert _scan("--allow", "cross.o", build("op_sel:[0,1] op_sel_hi:[1,0]", "across")).returncode == 1     # exact names only
    ok = _scan(build("", "plain"))
    assert ok.returncode == 0 and " 0 cross-half refused" in ok.stdout, ok.stdout[-2000:]


def test_scan_text_reads_op_sel_only():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_pk_cross_half as pk
    text = "\n".join(["0000000000000000 <k>:",
                      "\tv_pk_add_f32 v[4:5], v[0:1], v[2:3] op_sel:[0,1] op_sel_hi:[1,0]  // 000000000000: 00",
                      "\tv_pk_fma_f32 v[4:5], v[0:1], v[2:3], v[6:7] op_sel_hi:[1,0,1]  // 000000000008: 00",
                      "\tv_pk_mul_f32 v[4:5], v[0:1], v[2:3]  // 000000000010: 00"])
    refused, allowed = pk.scan_text(text, "x.o")
    assert len(refused) == 1 and "op_sel:[0,1]" in refused[0] and allowed == []
