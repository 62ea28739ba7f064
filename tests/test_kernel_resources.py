"""tools/kernel_resources.py -- the gate for edits of csrc/chain_common.h -- on a hand-written assembly file in the compiler's layout:
it reads the figures and counts, tells a pinned difference from a free one, and fails loudly on a file it cannot parse."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'kernel_resources.py')

ASM = '''\t.text
k1:                                     ; @k1
; %%bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
%s
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel k1
\t.end_amdhsa_kernel
\t.text
.Lfunc_end0:
; Kernel info:
; codeLenInByte = 16
; NumSgprs: 10
; NumVgprs: %d
; NumAgprs: 0
; ScratchSize: 0
; LDSByteSize: 1024 bytes/workgroup (compile time only)
; Occupancy: 2
\t.text
amdhsa.kernels:
  - .name:           k1
    .vgpr_spill_count: 0
'''


def run(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=60)


def write(tmp_path, name, body, vgprs=8):
    p = tmp_path / name
    p.write_text(ASM % (body, vgprs))
    return str(p)


def test_diff_tells_pinned_from_free(tmp_path):
    a = write(tmp_path, 'a.s', '\tv_fma_f32 v0, v1, v2, v3\n\ts_nop 0')
    same = write(tmp_path, 'b.s', '\ts_nop 0\n\tv_fma_f32 v0, v1, v2, v3\n\ts_nop 1')
    more = write(tmp_path, 'c.s', '\tv_fma_f32 v0, v1, v2, v3\n\tv_fma_f32 v0, v1, v2, v3\n\ts_nop 0')
    regs = write(tmp_path, 'd.s', '\tv_fma_f32 v0, v1, v2, v3\n\ts_nop 0', vgprs=9)
    r = run('--diff', a, same)
    assert r.returncode == 0 and 'free to differ: s_nop +1' in r.stdout
    r = run('--diff', a, more)
    assert r.returncode == 1 and 'PINNED DIFFER' in r.stdout and 'v_fma_f32 +1' in r.stdout
    r = run('--diff', a, regs)
    assert r.returncode == 1 and 'VGPR 8 -> 9' in r.stdout


def test_unparsable_assembly_is_an_error(tmp_path):
    empty = tmp_path / 'empty.s'
    empty.write_text('\t.text\n')
    assert run(str(empty)).returncode != 0
    assert run('--diff', str(empty), str(empty)).returncode != 0
    a = write(tmp_path, 'a.s', '\ts_nop 0')
    shifted = tmp_path / 'shifted.s'
    shifted.write_text(open(a).read().replace('; Kernel info:', '; Kernel information:'))
    assert run('--diff', a, str(shifted)).returncode != 0
