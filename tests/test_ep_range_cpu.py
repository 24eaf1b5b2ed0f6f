"""stk_ep_fits_buffer (csrc/ep_range.h): which tensors the GEMM epilogues of csrc/conv.hip address through 32-bit byte
offsets with bit 31 as the dead-element marker, and which keep the element code with 64-bit addresses.  The header is
plain C++; it is compiled into a small stand-alone program with the host compiler and run -- no GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include "ep_range.h"
int main() {
  const long GiB2 = 1L << 31;                       // bytes
  struct { long elems; bool fits; } cases[] = {
    {0, true}, {1, true},
    {128L * 128 * 32 * 32, true},                   // a 32x32 activation at batch 128: 64 MiB
    {GiB2 / 4 - 1, true},                           // the last element's offset is 2^31 - 8
    {GiB2 / 4, false},                              // exactly 2 GiB: offset 2^31 - 4 is still free of bit 31, the byte COUNT is not
    {GiB2 / 4 + 1, false},
    {0x7fffffffL, false},                           // the most elements the host side admits
    {1L << 40, false}, {-1, false},
  };
  int bad = 0;
  for (auto& c : cases)
    if (stk_ep_fits_buffer(c.elems) != c.fits) { std::printf("elems %ld: want %d\n", c.elems, (int)c.fits); ++bad; }
  // every tensor that fits keeps each byte offset, and the resource's byte count, below bit 31
  for (long e = GiB2 / 4 - 3; e < GiB2 / 4 + 3; ++e)
    if (stk_ep_fits_buffer(e) && !(e * 4 < GiB2)) { std::printf("elems %ld fits but its byte count has bit 31\n", e); ++bad; }
  return bad;
}
'''


def test_selection_predicate(tmp_path):
  cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
  if cxx is None:
    pytest.fail('no host C++ compiler to build the stand-alone program with')
  src = tmp_path / 'ep_range_main.cpp'
  src.write_text(PROGRAM)
  exe = tmp_path / 'ep_range_main'
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'soft-truncation_amd', 'csrc'),
                         str(src), '-o', str(exe)])
  r = subprocess.run([str(exe)], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout
