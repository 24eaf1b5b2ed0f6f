// ep_range.h -- which addressing form a GEMM epilogue of conv.hip takes for one tensor.  Plain C++ (host and device), so that
// the rule can be compiled and tested without a GPU (tests/test_ep_range_cpu.py).
//
// The epilogues address their outputs, residuals and old gradients through buffer resources: a wave-uniform base, a 32-bit
// per-lane BYTE offset, and bit 31 of that offset as the "dead element" marker (the range check then returns 0 for a load
// and drops a store).  That form can reach a tensor only if every byte offset into it stays below bit 31; the host side
// admits tensors of up to 2^31 - 1 ELEMENTS, four times as much.  A tensor that does not fit takes the element-wise path
// with 64-bit addresses instead -- chosen per tensor, by this one wave-uniform test.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STK_EP_HD __host__ __device__
#else
#define STK_EP_HD
#endif

// true: all of a tensor of `elems` floats lies below byte offset 2^31 (buffer form); false: the 64-bit element path
#ifdef STK_EP_BUFFER_FORM_ONLY
// Analysis builds only (tools/epilogue_isa.py -DSTK_EP_BUFFER_FORM_ONLY): the element path folds away, so that the table
// counts the instructions of the buffer form alone.  Never defined for libstk.so.
STK_EP_HD inline bool stk_ep_fits_buffer(long) { return true; }
#else
STK_EP_HD inline bool stk_ep_fits_buffer(long elems) { return elems >= 0 && elems < (1L << 29); }
#endif
