// Device primitives shared by the gfx950 kernels of libgrr.so: vector types, row loads / stores, DPP lane
// shifts, the wave / workgroup sums of the fixed-order reductions and the LDS-DMA wrappers.  Everything is
// __forceinline__: a kernel that uses a helper compiles to the code it had with a private copy.
#pragma once

#include "grr_common.h"

namespace grr {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) float* lds_f32_t;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// V adjacent floats as one load / store
template <int V> struct VecT;
template <> struct VecT<1> { typedef float type; };
template <> struct VecT<2> { typedef f32x2 type; };
template <> struct VecT<4> { typedef f32x4 type; };
template <> struct VecT<8> { typedef f32x8 type; };

template <int V>
__device__ __forceinline__ void row_load(float (&d)[V], const float* p) {
  const typename VecT<V>::type t = *reinterpret_cast<const typename VecT<V>::type*>(p);
  if constexpr (V == 1) {
    d[0] = t;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) d[j] = t[j];
  }
}
template <int V>
__device__ __forceinline__ void row_store(float* p, const float (&v)[V]) {
  typename VecT<V>::type t;
  if constexpr (V == 1) {
    t = v[0];
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) t[j] = v[j];
  }
  *reinterpret_cast<typename VecT<V>::type*>(p) = t;
}

// ---------------------------------------------------------------------------
// DPP lane shifts: the value of lane - 1 / lane + 1 (0 past the wave's ends).  Cross-lane reads must
// execute with the whole wave active: a DPP read of a lane that is masked off returns 0.
// ---------------------------------------------------------------------------

// Pinned: the empty asm fixes each result at its definition, so the compiler cannot sink the
// v_mov_b32_dpp into a divergent branch (it turned `c > 0 ? lane_prev(v) : 0` into an exec-masked branch
// before this was added).  Use these wherever the result feeds a lane-dependent select.
__device__ __forceinline__ float lane_prev(float v) {
  float r = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, true));
  asm volatile("" : "+v"(r));
  return r;
}
__device__ __forceinline__ float lane_next(float v) {
  float r = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xF, 0xF, true));
  asm volatile("" : "+v"(r));
  return r;
}
// Unpinned: no asm statement, which would end the scheduling region (feature_edge.hip spreads its conv
// MFMAs over the edge arithmetic).  DPP moves are convergent, so they are never sunk into a branch by
// themselves; use these only in straight-line code with the whole wave active.
__device__ __forceinline__ float lane_prev_free(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, true));
}
__device__ __forceinline__ float lane_next_free(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xF, 0xF, true));
}
// every lane of a quad takes the quad's element E (unpinned)
template <int E>
__device__ __forceinline__ float quad_bcast(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), E * 0x55, 0xF, 0xF, true));
}

// ---------------------------------------------------------------------------
// Sums for the fixed-order reductions (grr_common.h)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// one partial per block of NT threads: wave sums -> LDS -> thread 0 adds them in wave order and stores the
// block's slot.  Every thread of the block must call it (it synchronises); consecutive calls reuse the
// LDS slots safely.
template <int NT>
__device__ __forceinline__ void block_red_put(const Red& r, int idx, uint32_t slot, float v) {
  __shared__ float red[NT / 64];
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    red_put(r, idx, slot, t);
  }
}
// slot of block (blockIdx.x, blockIdx.y) of a (chunks, B * per) grid: one per (b, chunk)
__device__ __forceinline__ uint32_t chunk_slot(int per) {
  return (uint32_t)(blockIdx.y / per) * gridDim.x + blockIdx.x;
}

// ---------------------------------------------------------------------------
// LDS-DMA (global -> LDS without registers): lane l's bytes land at the wave-uniform LDS base + size * l
// ---------------------------------------------------------------------------

// 16 bytes per lane, builtin form: the compiler orders it (lgkmcnt(0) / vmcnt(0) before later LDS reads)
__device__ __forceinline__ void dma16(const void* src, float* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(src, (lds_ptr_t)lds_wave_base, 16, 0, 0);
}
// The same 16-byte LDS-DMA as an asm statement.  hipcc answers every LDS-DMA builtin with full waits at
// all later LDS reads (it cannot order the DMA's LDS write against them), which drains whatever loads a
// kernel keeps in flight; a kernel that orders its ring itself (counted vmcnt + barrier) issues the DMA
// opaquely and keeps the compiler's counted waits.  The compiler does not count these operations: its
// own waits stay correct with them in flight (vmcnt retires loads in order: a wait only gets stricter),
// but nothing waits for them except the kernel's own counted vmcnt.
__device__ __forceinline__ void dma16_opaque(const void* src, const float* lds_wave_base) {
  const uint32_t m0v = (uint32_t)(uintptr_t)(lds_f32_t)lds_wave_base;
  asm volatile("global_load_lds_dwordx4 %0, off" ::"v"(src), "{m0}"(__builtin_amdgcn_readfirstlane(m0v)) : "memory");
}
// 4 bytes per lane, opaque
__device__ __forceinline__ void dma_dword(const float* src, float* lds_wave_base) {
  const uint32_t m0v = (uint32_t)(uintptr_t)(lds_f32_t)lds_wave_base;
  asm volatile("global_load_lds_dword %0, off" ::"v"(src), "{m0}"(__builtin_amdgcn_readfirstlane(m0v)) : "memory");
}
// 16 bytes per lane, opaque, scalar base + a loop-invariant per-lane byte offset: the VGPR operand is never
// rewritten while DMAs that read it are in flight (a rewritten address VGPR drew compiler vmcnt(0) waits
// inside the issue loop)
__device__ __forceinline__ void dma_row16(const float* sbase, uint32_t voff, float* lds_dst) {
  const uint32_t m0v = (uint32_t)(uintptr_t)(lds_f32_t)lds_dst;
  asm volatile("global_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "{m0}"(__builtin_amdgcn_readfirstlane(m0v))
               : "memory");
}

// ---------------------------------------------------------------------------
// The counter-based normals of grr_patch_batch and grr_patch_raw_batch (include/grr.h): a function of (seed, sample
// id, element)
// ---------------------------------------------------------------------------

// Philox4x32-10 (Salmon et al., SC'11; Random123's constants)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&x)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// the two float64 normals of a word pair: u = (x + 0.5) 2^-32 in (0, 1), Box-Muller
__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, double* za, double* zb) {
  const double u0 = ((double)xa + 0.5) * 0x1p-32, u1 = ((double)xb + 0.5) * 0x1p-32;
  const double r = sqrt(-2.0 * log(u0)), th = 6.283185307179586 * u1;
  *za = r * cos(th);
  *zb = r * sin(th);
}

struct NoiseKey {
  uint32_t id_lo, id_hi, seed_lo, seed_hi;
};

// the 4 normals of block b = e / 4 of a sample
__device__ __forceinline__ void normals4(uint32_t b, const NoiseKey& k, double (&z)[4]) {
  uint32_t x[4];
  philox4x32_10(b, 0u, k.id_lo, k.id_hi, k.seed_lo, k.seed_hi, x);
  box_muller(x[0], x[1], &z[0], &z[1]);
  box_muller(x[2], x[3], &z[2], &z[3]);
}

// the normal of element e alone (a lane whose 4 C elements do not start on a block)
__device__ __forceinline__ double normal_at(uint32_t e, const NoiseKey& k) {
  uint32_t x[4];
  philox4x32_10(e >> 2, 0u, k.id_lo, k.id_hi, k.seed_lo, k.seed_hi, x);
  const bool hi = (e & 2u) != 0;
  double za, zb;
  box_muller(hi ? x[2] : x[0], hi ? x[3] : x[1], &za, &zb);
  return (e & 1u) ? zb : za;
}

}  // namespace grr
