// povar_kernels_ck_parts.hpp -- what the camera-chunk kernels share: e0_ck (povar_kernels_ck.hpp), e0_ck_h (.._ck_joint.hpp),
// e0_ck_f32 (.._ck_f32.hpp), e0_ck_det / e0_ck_h_det (.._ck_det.hpp).  Pieces, not a walker: every kernel keeps its batch loop
// and phases, the order of its requests, its `asm volatile("" : "+v"(lane))` fences and its arithmetic.  Here: the slot word
// (ck_slot), the row walk (ck_walk_rows), the row stream (CkRowStream + payloads; aliases CkStream, CkStreamH, Ck32Stream),
// a tile's header (CkTile: e0_ck_h and e0_ck_f32 -- in e0_ck and the det pair it moved s_waitcnt counts, registers and
// e0_ck's s_waitcnt order, profiles/ck_parts_isa.txt: those keep their own text) and a lane's DECODED metadata (CkLaneMeta:
// e0_ck_f32; e0_ck and e0_ck_h carry the raw words across their barriers and decode at first use, povar_kernels_ck.hpp).
// Included by povar_kernels_ck.hpp behind WAVE, CK_NONE, CkP, ck_rank / ck_seg and ck_unpack_uv, never on its own.  Every
// function is __forceinline__ and every member a value: tile headers stay in SGPRs, the row buffers in VGPRs.
//
// INVARIANTS of the row stream (the one place they are stated):
//   * D rows are in flight ahead of the row being worked on, in D STATICALLY indexed buffers: the walk is unrolled by D, so
//     that a row's loads really have D steps to land.  (A rolled loop with a shift register of D buffers was built first: the
//     register moves of step j + 1 touch what step j has just requested, so every row waited for its predecessor's loads
//     whatever D was -- s_waitcnt vmcnt(0) at the top of the loop, 1400 cycles per row on the way back.)
//   * D is even: the two landmark slots of an li word then sit at a static shift.  (D = 1: the cold loops, which keep nothing
//     in flight.)
//   * a request past the tile's end re-reads its last row -- a cache hit --, so that every step issues the same loads and the
//     wait counters can be exact: with loads under `if (j < h)` the compiler waited for all but the newest load, i.e. for the
//     row it had requested one step earlier.
//   * the rows of a tile are requested after everything else of their phase.  The wait counters retire in issue order; with
//     younger loads pending behind the rows, the compiler's merge of the loop-entry and back-edge states at the head of the row
//     loop came out as s_waitcnt vmcnt(0): every row waited for the row requested one step earlier.
#pragma once

namespace povar {

typedef unsigned __attribute__((ext_vector_type(2))) ck_u2;

// ---- the slot word: two 16-bit words per li entry, rows 2 n and 2 n + 1 of a tile; CkP::li says what a word addresses
__device__ __forceinline__ uint32_t ck_slot(uint32_t word, int j) { return (word >> (16 * (j & 1))) & CK_NONE; }  // (CK_NONE: ck_layout.hpp)

// ---- the rows of one tile (h >= 1): step n of the walk is row n (DIR = +1) or row h - 1 - n (DIR = -1: the way back starts
// with the rows the way forward read last, the ones most likely still in the XCD's L2); buffer n % D holds it.  step(row,
// buffer) works on the row and requests row + DIR * D into the buffer it has just emptied.
template <int D, int DIR, class Step>
__device__ __forceinline__ void ck_walk_rows(int h, Step&& step) {
  int n0 = 0;
#pragma nounroll
  for (; n0 + D <= h; n0 += D) {
#pragma unroll
    for (int i = 0; i < D; ++i) step(DIR > 0 ? n0 + i : h - 1 - (n0 + i), i);
  }
#pragma unroll
  for (int i = 0; i < D - 1; ++i)  // the last h % D rows
    if (n0 + i < h) step(DIR > 0 ? n0 + i : h - 1 - (n0 + i), i);
}

// ---- the row stream.  Buffer descriptors of the row arrays (wave-uniform: built once per kernel from kernel arguments): the
// rows are read through them -- descriptor in SGPRs + the lane's constant 32-bit byte offset + the row's byte offset as the
// scalar offset: no VALU instruction per load (a flat load took a 64-bit add each, two per row and pass in loops that are
// VALU-bound).
struct CkRows {
  __amdgpu_buffer_rsrc_t uv, li, w;  // (uv: step 1; w: step 2 with a robust norm)
};

// What a row holds beside its slot word.  A payload has D buffers, clear(i), request(R, row, lane, i) -- row: the row's
// number in the row arrays -- and SLOT_FIRST: whether the slot word is requested before the payload (the order of issue is
// the order the wait counters retire in: each kernel keeps the one it was measured with).
// step 1, fp64: the image point, plain (double2) or packed (ck_layout.hpp: ck_pack_uv).  Packed words are decoded when the
// row is worked on (get), not when it is requested: a decode at the request makes the wavefront wait for the row there, and
// e0_ck requests a batch's first rows in front of the barrier that ends the batch before.
template <int D, bool PK>
struct CkUvRows {
  static constexpr bool SLOT_FIRST = false;
  double2 uv[D];
  unsigned pk[D][2];
  __device__ __forceinline__ void clear(int i) {
    uv[i] = make_double2(0, 0);
    pk[i][0] = pk[i][1] = 0;
  }
  __device__ __forceinline__ void request(const CkRows& R, unsigned row, unsigned lane, int i) {
    const unsigned ro = row * (unsigned)(WAVE * 16);
    if (PK) {  // 8 bytes per observation
      const ck_u2 a = __builtin_amdgcn_raw_buffer_load_b64(R.uv, lane * 8u, ro >> 1, 0);
      pk[i][0] = a.x;
      pk[i][1] = a.y;
    } else {
      const ck_u4 a = __builtin_amdgcn_raw_buffer_load_b128(R.uv, lane * 16u, ro, 0);
      uv[i] = make_double2(__longlong_as_double(((long long)a.y << 32) | a.x), __longlong_as_double(((long long)a.w << 32) | a.z));
    }
  }
  __device__ __forceinline__ double2 get(int i) const { return PK ? make_double2(ck_unpack_uv(pk[i][0]), ck_unpack_uv(pk[i][1])) : uv[i]; }
};
// step 2: the robust weight, or nothing (the operator does not read the image points: povar_kernels_ck_joint.hpp)
template <int D, bool ROBUST>
struct CkWeightRows {
  static constexpr bool SLOT_FIRST = true;
  double rw[D];
  __device__ __forceinline__ void clear(int i) { rw[i] = 1.0; }
  __device__ __forceinline__ void request(const CkRows& R, unsigned row, unsigned lane, int i) {
    if (ROBUST) {
      const ck_u2 b = __builtin_amdgcn_raw_buffer_load_b64(R.w, lane * 8u, row * (unsigned)(WAVE * 8), 0);
      rw[i] = __longlong_as_double(((long long)b.y << 32) | b.x);
    }
  }
};
// step 1, fp32: the image point as float2, or packed: k micro-units (the packing verified that k * 10^-6 is the file's number)
__device__ __forceinline__ float ck32_unpack(unsigned k) { return (float)(int)k * 1e-6f; }
template <int D, bool PK>
struct CkUv32Rows {
  static constexpr bool SLOT_FIRST = false;
  float2 uv[D];
  __device__ __forceinline__ void request(const CkRows& R, unsigned row, unsigned lane, int i) {
    const ck_u2 a = __builtin_amdgcn_raw_buffer_load_b64(R.uv, lane * 8u, row * (unsigned)(WAVE * 8), 0);
    if (PK) uv[i] = make_float2(ck32_unpack(a.x), ck32_unpack(a.y));
    else uv[i] = make_float2(__uint_as_float(a.x), __uint_as_float(a.y));
  }
};

template <int D, class Payload>
struct CkRowStream : Payload {
  static_assert(D == 1 || D % 2 == 0, "the slots of an li word sit at a static shift only with an even depth");
  uint32_t w[D];  // the slot words (ck_slot)
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      Payload::clear(i);
      w[i] = 0xffffffffu;
    }
  }
  // buffer i <- row j of the tile (clamped into the tile)
  __device__ __forceinline__ void load(const CkRows& R, int row0, int li0, int j, int h, int lane, int i) {
    j = j < 0 ? 0 : (j >= h ? h - 1 : j);
    const unsigned ul = (unsigned)lane, lo = (unsigned)(li0 + (j >> 1)) * (unsigned)(WAVE * 4);
    if (Payload::SLOT_FIRST) w[i] = __builtin_amdgcn_raw_buffer_load_b32(R.li, ul * 4u, lo, 0);
    Payload::request(R, (unsigned)(row0 + j), ul, i);
    if (!Payload::SLOT_FIRST) w[i] = __builtin_amdgcn_raw_buffer_load_b32(R.li, ul * 4u, lo, 0);
  }
  // the first D steps of a walk (ck_walk_rows<D, DIR>)
  template <int DIR>
  __device__ __forceinline__ void start(const CkRows& R, int row0, int li0, int h, int lane) {
#pragma unroll
    for (int i = 0; i < D; ++i) load(R, row0, li0, DIR > 0 ? i : h - 1 - i, h, lane, i);
  }
};
// (ROBUST of CkStream: the weight is recomputed, not a row array -- the parameter names the instantiation, nothing else)
template <int D, bool ROBUST, bool PK = false> using CkStream = CkRowStream<D, CkUvRows<D, PK>>;
template <int D, bool ROBUST> using CkStreamH = CkRowStream<D, CkWeightRows<D, ROBUST>>;
template <int D, bool PK> using Ck32Stream = CkRowStream<D, CkUv32Rows<D, PK>>;  // (never cleared: every walk starts it)

// ---- a tile's header (CkP::tile: first row, height, flags, first li row): wave-uniform values, in SGPRs
struct CkTile {
  int row0, h, fl, li0;
  // the tile table through the scalar cache (constant address space + wave-uniform index)
  typedef const int __attribute__((address_space(4))) * table_p;
  __device__ static __forceinline__ table_p table(const CkP& k) { return (table_p)(uintptr_t)k.tile; }
  __device__ static __forceinline__ CkTile load(table_p tiles, int t) {
    return CkTile{tiles[4 * t], tiles[4 * t + 1], tiles[4 * t + 2], tiles[4 * t + 3]};
  }
  // ... from a header the kernel has loaded itself (e0_ck_f32: one vector load of the wave-uniform address)
  __device__ static __forceinline__ CkTile of(int4 v) { return CkTile{v.x, v.y, v.z, v.w}; }
};

// ---- a lane's metadata in a tile (CkP::lane_meta): rank of its camera (< 0: empty lane), first | last << 8 lane of the run
// that shares its accumulator, accumulator slot (< 0: ~(partial record of a chunk without one)).  Per-lane values.
struct CkLaneMeta {
  int rank, seg, acc;
  __device__ static __forceinline__ CkLaneMeta load(const CkP& k, int t, int lane) {
    const int2 m = k.lane_meta[(size_t)t * WAVE + lane];
    return CkLaneMeta{ck_rank(m.x), ck_seg(m.x), m.y};
  }
  // the rank alone (the way forward: one 4-byte load)
  __device__ static __forceinline__ int rank_of(const CkP& k, int t, int lane) { return ck_rank(k.lane_meta[(size_t)t * WAVE + lane].x); }
};

}  // namespace povar
