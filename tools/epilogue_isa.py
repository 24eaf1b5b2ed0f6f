#!/usr/bin/env python
"""What hipcc made of the GEMM epilogues: per kernel of conv.hip, everything behind the last v_mfma is counted.
CPU only (hipcc cross-compiles conv.hip to gfx950 assembly with the flags of csrc/Makefile).

  full waits   s_waitcnt with vmcnt(0): every outstanding load AND store must be acknowledged
  cnt waits    s_waitcnt with vmcnt(N > 0): a counted wait, the loads behind it stay in flight
  stores/loads global_ / buffer_ / flat_ memory instructions
  exec br      s_cbranch_execz / s_cbranch_execnz: one per exec-masked block (`if (ok) store`)
  unif br      s_cbranch_scc* / s_cbranch_vcc*: wave-uniform option branches

usage: python tools/epilogue_isa.py [--src conv.hip] [-D MACRO ...] [name filter ...]
Default filters: the kernels that finish through EpFwd / EpDgrad / EpSlab / EpWgrad on the split path."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'soft-truncation_amd', 'csrc')
# hipcc as csrc/Makefile finds it: $HIPCC, else the one on PATH, else the default ROCm location
HIPCC = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
HAZARD_FLAGS = ['-fno-slp-vectorize', '-Xclang', '-target-feature', '-Xclang', '-packed-fp32-ops']
DEFAULT = ['x2d::gemm_halo_kernel<32, EpFwd, 1>', 'x2d::gemm_halo_kernel<16, EpFwd, 1>', 'x2d::gemm_halo_kernel<64, EpFwd, 1>',
           'x2d::gemm_halo_kernel<32, EpDgrad, 1>', 'x2d::gemm_halo_kernel<16, EpDgrad, 1>',
           'x2d::gemm_kernel<9, 128, EpFwd', 'x2d::gemm_kernel<1, 128, EpFwd', 'x2d::gemm_kernel<9, 128, EpDgrad',
           'x2d::gemm_kernel<1, 128, EpDgrad', 'x2d::gemm_kernel<9, 128, EpSlab', 'x2d::gemm_kernel<1, 128, EpSlab',
           'x2::gemm_kernel<x2::ActLoader<true, 1>, EpFwd', 'x2::gemm_kernel<x2::ActLoader<false, 1>, EpDgrad',
           'x2::wgemm_kernel<x2::RowsU<false, false>, x2::RowsU<true, true>, EpWgrad']
PATTERNS = [('full waits', re.compile(r'^s_waitcnt\b.*vmcnt\(0\)')),
            ('cnt waits', re.compile(r'^s_waitcnt\b.*vmcnt\([1-9]\d*\)')),
            ('stores', re.compile(r'^(global|buffer|flat)_store_')),
            ('loads', re.compile(r'^(global|buffer|flat)_load_')),
            ('exec br', re.compile(r'^s_cbranch_exec')),
            ('unif br', re.compile(r'^s_cbranch_(scc|vcc)'))]


def assembly(src, defines):
  with tempfile.TemporaryDirectory() as tmp:
    out = os.path.join(tmp, 'conv.s')
    r = subprocess.run([HIPCC, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', *HAZARD_FLAGS,
                        *['-D' + d for d in defines], '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.dirname(src),
                        '-S', '--cuda-device-only', src, '-o', out], capture_output=True, text=True)
    if r.returncode != 0:
      sys.stderr.write(r.stderr)
      sys.exit(f'{HIPCC} failed on {src} (exit {r.returncode})')
    return open(out).read()


def kernels(text):
  """(mangled name, body lines, codeLenInByte, NumVgprs) of every function of the assembly"""
  cur, body = None, []
  for line in text.splitlines():
    m = re.match(r'^(_Z\w+):', line)
    if m:
      cur, body = m.group(1), []
      continue
    if cur is None:
      continue
    body.append(line.strip())
    m = re.match(r'^; NumVgprs: (\d+)', line)
    if m:
      size = next((int(x.split('=')[1]) for x in body if x.startswith('; codeLenInByte')), 0)
      yield cur, body, size, int(m.group(1))
      cur = None


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--src', default=os.path.join(CSRC, 'conv.hip'))
  ap.add_argument('-D', dest='defines', action='append', default=[])
  ap.add_argument('filters', nargs='*')
  args = ap.parse_args()
  filters = args.filters or DEFAULT
  rows = list(kernels(assembly(args.src, args.defines)))
  names = subprocess.run(['c++filt'], input='\n'.join(r[0] for r in rows), capture_output=True, text=True).stdout.splitlines()
  print(f"{'kernel (behind its last v_mfma)':<100} " + ' '.join(f'{h:>10}' for h, _ in PATTERNS) + f" {'code bytes':>10} {'VGPRs':>6}")
  for (mangled, body, size, vgprs), name in zip(rows, names):
    name = re.sub(r'\(anonymous namespace\)::', '', name)
    name = name[:name.index('(')] if '(' in name else name
    name = re.sub(r'^void ', '', name)
    if not any(f in name for f in filters):
      continue
    last = max((i for i, x in enumerate(body) if x.startswith('v_mfma')), default=-1)
    if last < 0:
      continue
    tail = body[last + 1:]
    counts = [sum(1 for x in tail if pat.match(x)) for _, pat in PATTERNS]
    print(f'{name[:100]:<100} ' + ' '.join(f'{c:>10}' for c in counts) + f' {size:>10} {vgprs:>6}')


if __name__ == '__main__':
  sys.exit(main())
