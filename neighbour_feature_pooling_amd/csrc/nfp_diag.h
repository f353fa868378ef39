// nfp_diag.h — diagnostic build only (-DNFP_STAMPS, scripts/diag_stamps.py): thread 0 of every workgroup records
// {shader clock, 100 MHz wall clock} at phase boundaries into a buffer nothing else reads.  Never part of the
// product library: nfp_common.h includes this file only under NFP_STAMPS.
#pragma once
// (included from inside namespace nfp)
__constant__ unsigned long long* nfp_stamp_buf = nullptr;
// Every translation unit whose kernels stamp has its own copy of that pointer, and (at file scope) exports a setter for it;
// nfp_hip.hip::nfp_debug_set_stamp_buffer calls them all.
#define NFP_STAMP_SETTER(unit)                                                                      \
  extern "C" int nfp_debug_set_stamp_buffer_##unit(void* dev_ptr) {                                 \
    unsigned long long* p = (unsigned long long*)dev_ptr;                                           \
    return hipMemcpyToSymbol(HIP_SYMBOL(nfp::nfp_stamp_buf), &p, sizeof(p)) == hipSuccess ? 0 : -3; \
  }
// The buffer pointer is read ONCE, by a scalar load (constant address space: its wait is on lgkmcnt and does not
// cover vector loads in flight — fwd_band / bwd_fast read it BEHIND their first requests, below); a stamp is then one
// s_memtime/s_memrealtime pair and two stores, with no vmcnt wait, so loads in flight stay in flight.
#define NFP_STAMP_INIT() unsigned long long* nfp_sb_ = nfp_stamp_buf
#define NFP_STAMP(id)                                                                        \
  do {                                                                                       \
    if ((threadIdx.x | threadIdx.y | threadIdx.z) == 0 && nfp_sb_) {                                                       \
      unsigned long long wg = blockIdx.x + (unsigned long long)gridDim.x * blockIdx.y;       \
      nfp_sb_[(wg * 16 + (id)) * 2] = __builtin_amdgcn_s_memtime();                         \
      nfp_sb_[(wg * 16 + (id)) * 2 + 1] = __builtin_amdgcn_s_memrealtime();                 \
    }                                                                                        \
  } while (0)
// fwd_band / bwd_fast: the entry stamp is a read of the two clocks into registers at the kernel's first instruction
// (NFP_STAMP_ENTRY — no pointer, no memory request); the buffer pointer is loaded and the pair stored as stamp 0 behind the
// kernel's first requests (NFP_STAMP_INIT_ENTRY), so that the stamp's own pointer load does not stand in front of what it measures.
#define NFP_STAMP_ENTRY()                                              \
  const unsigned long long nfp_c0_ = __builtin_amdgcn_s_memtime();     \
  const unsigned long long nfp_r0_ = __builtin_amdgcn_s_memrealtime()
#define NFP_STAMP_INIT_ENTRY()                                                               \
  NFP_STAMP_INIT();                                                                          \
  do {                                                                                       \
    if ((threadIdx.x | threadIdx.y | threadIdx.z) == 0 && nfp_sb_) {                         \
      unsigned long long wg = blockIdx.x + (unsigned long long)gridDim.x * blockIdx.y;       \
      nfp_sb_[wg * 16 * 2] = nfp_c0_;                                                        \
      nfp_sb_[wg * 16 * 2 + 1] = nfp_r0_;                                                    \
    }                                                                                        \
  } while (0)
