// tile.h -- what the matrix-core line kernels share (device-inline; host launchers use the geometry constants only):
// cheb_sweep_kernel (sweep.hip), vec1_body / vec4_body (sweep_vec.hip), cheb_fused_kernel (fused.hip), cheb_fused4_kernel (fused4.hip).
// The rule: a helper is used where the kernel's machine code stays what it was (profiles/tile_refactor/isa_compare.txt); where hipcc
// schedules a kernel differently through a helper, the kernel keeps those lines and says so.
// All of them: 512 threads = 8 waves; wave w owns the 16 output rows of m-tile w % MTP and the lines of wave group w / MTP; a tile of
// NT lines sits parity-split (E, O) in LDS; v_mfma_f64_16x16x4_f64 chains run over it with the matrix halves in registers.
#pragma once
#include <hip/hip_runtime.h>

namespace chebhip {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef unsigned u32;
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

// Tile geometry of a kernel with KS k-steps (lines of up to 8 KS points) and a loader that moves LB = 8 or 16 bytes per slot.
template <int KS, bool JFAST, int LB = 16>
struct TileGeom {
  static constexpr int MTP = KS / 4;                      // m-tiles of 16 output rows (padded)
  static constexpr int NG = 8 / MTP;                      // wave groups along the line index
  static constexpr int HP = 4 * KS;                       // padded half length
  static constexpr int NSUB = (KS >= 16) ? 2 : 1;         // 16-line sub-tiles per wave per tile
  static constexpr int NT = 16 * NG * NSUB;               // lines per tile
  // Pitch of a line of the JFAST tile image in LDS.  ODD: the MFMA operand reads -- lane (l16, kq) reads points kq + 4k, kq + 4k + 4 of
  // line l16 as one ds_read2_b64 -- are free of bank conflicts; with the pitch = 2 mod 32 of rounds 1-5 every such read is a 2-way
  // conflict (tools/lds_probe.hip under --pmc, profiles/r06_lds_probe.txt: SQ_LDS_BANK_CONFLICT = half of SQ_LDS_IDX_ACTIVE at pitch
  // 130, 0 at 129, three quarters at 132 -- the 8.26 M conflict cycles of the JFAST launch in every counter record since round 3).  The
  // price: lines start on 8-byte boundaries only, so a parity split parks its 16-byte pieces as ds_write2_b64 instead of ds_write_b128.
  static constexpr int LDJ = HP + 1;
  static constexpr int LDS_ELEMS = JFAST ? NT * LDJ : HP * NT;   // doubles of one image (E or O) of a tile
  static constexpr int PER = LB / 8;                      // doubles per loader slot
  static constexpr int ITEMS = HP * NT / PER / 512;       // loader slots per thread per tile
  static constexpr int CH = ITEMS / NSUB;                 // slots per chunk (one chunk rides under one sub-tile)
  // loader slot 0 of thread tid: JFAST points PER a .. of line b, COLFAST lines PER a .. of point b, with a = tid % LD_W, b = tid / LD_W
  // (a slot adds QSTEP to b).  The kernels write these out: behind a function hipcc folds the index arithmetic in another order
  static constexpr int LD_W = (JFAST ? HP : NT) / PER;
  static constexpr int QSTEP = 512 / LD_W;                // line step (JFAST) / point step (COLFAST) between two slots of a thread
  static constexpr int LDS_QSTEP = JFAST ? QSTEP * LDJ : QSTEP * NT;   // (QSTEP even -> swizzle parity unchanged)
  static constexpr int KSTR = JFAST ? 4 : 4 * NT;         // LDS stride of one k-step
  // KS = 32, 16-byte kernels: the last NFL odd-half fragments of a wave live in LDS behind the tile images, KR stay in registers
  static constexpr int NFL = (KS == 32) ? (JFAST ? 7 : 8) : 0;
  static constexpr int KR = KS - NFL;
  static constexpr int LDS_DOUBLES = 4 * LDS_ELEMS + 8 * NFL * 64;   // two (E, O) image pairs plus those fragments
  static_assert(LB == 8 || LB == 16, "8- or 16-byte loader slots");

  // LDS index of (point i, line n) in an image: COLFAST rows are points, with the line index swizzled by the point's parity
  static __device__ __forceinline__ int at(int i, int n) { return JFAST ? n * LDJ + i : i * NT + (n ^ ((i & 1) << 4)); }
  // first MFMA operand of lane (l16, kq) for the 16 lines from nb on; k-step k adds k KSTR
  static __device__ __forceinline__ int frag(int nb, int l16, int kq) { return JFAST ? (nb + l16) * LDJ + kq : kq * NT + ((nb + l16) ^ ((kq & 1) << 4)); }
};

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt(0): every
// wave would wait at each tile boundary for its own prefetch loads and result stores, which
// serialises the HBM stream with the MFMA phases.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// XCD-aware tile walk of workgroup bid of nblk: workgroups b and b+8 share an XCD (and its L2).  Give each XCD one
// contiguous range of tiles and let its CUs take neighbouring tiles at the same time, so that a
// 128-B line straddled by two neighbouring row pieces is fetched from HBM once, not once per XCD.
// The workgroup walks first(), first() + t_step, ... < t_hi; rank(): its place among the workgroups of its XCD.
// (vec4_body, cheb_fused4_kernel; cheb_sweep_kernel, cheb_fused_kernel and vec1_body write the same five lines out.)
struct TileWalk {
  u32 bid, nxcd, t_lo, t_hi, t_step;
  __device__ __forceinline__ u32 rank() const { return bid / nxcd; }
  __device__ __forceinline__ u32 first() const { return t_lo + bid / nxcd; }
};
__device__ __forceinline__ TileWalk tile_walk(u32 bid, u32 nblk, u32 ntiles) {
  const u32 nxcd = (nblk % 8 == 0) ? 8u : 1u;
  const u32 t_per = (ntiles + nxcd - 1) / nxcd;
  const u32 t_lo = (bid % nxcd) * t_per;
  const u32 t_hi = (t_lo + t_per < ntiles) ? t_lo + t_per : ntiles;
  return TileWalk{bid, nxcd, t_lo, t_hi, nblk / nxcd};
}

// The two accumulator chains (even and odd half) of one 16-line sub-tile: KS k-steps in groups of two, operands at fE / fO + k KSTR.
// ae(k) / ao(k): matrix fragment k of this wave's m-tile; the matrix is the A operand (COLFAST: rows = outputs, columns = lines) or
// the B operand (JFAST: rows = lines, columns = outputs).  The fragment reads run one group ahead and a fence keeps them ABOVE the
// MFMAs of the group before (hipcc otherwise sinks them to just before their use and every group starts with an exposed LDS round
// trip).  hook(g) runs behind the fence of group g: where a kernel issues its loads / parks its prefetch inside the chain.
template <int KS, bool JFAST, int KSTR, class AE, class AO, class HOOK>
__device__ __forceinline__ void mfma_chain(const double *fE, const double *fO, v4d &ce, v4d &co, AE &&ae, AO &&ao, HOOK &&hook) {
  double fb[2][4];
  fb[0][0] = fE[0]; fb[0][1] = fE[KSTR]; fb[0][2] = fO[0]; fb[0][3] = fO[KSTR];
#pragma unroll
  for (int g = 0; g < KS / 2; g++) {
    const int cb = g & 1, nbuf = cb ^ 1;
    if (g + 1 < KS / 2) {
      fb[nbuf][0] = fE[(2 * g + 2) * KSTR]; fb[nbuf][1] = fE[(2 * g + 3) * KSTR];
      fb[nbuf][2] = fO[(2 * g + 2) * KSTR]; fb[nbuf][3] = fO[(2 * g + 3) * KSTR];
    }
    __builtin_amdgcn_sched_barrier(0);
    hook(g);
    if (!JFAST) {
      ce = __builtin_amdgcn_mfma_f64_16x16x4f64(ae(2 * g), fb[cb][0], ce, 0, 0, 0);
      co = __builtin_amdgcn_mfma_f64_16x16x4f64(ao(2 * g), fb[cb][2], co, 0, 0, 0);
      ce = __builtin_amdgcn_mfma_f64_16x16x4f64(ae(2 * g + 1), fb[cb][1], ce, 0, 0, 0);
      co = __builtin_amdgcn_mfma_f64_16x16x4f64(ao(2 * g + 1), fb[cb][3], co, 0, 0, 0);
    } else {
      ce = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[cb][0], ae(2 * g), ce, 0, 0, 0);
      co = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[cb][2], ao(2 * g), co, 0, 0, 0);
      ce = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[cb][1], ae(2 * g + 1), ce, 0, 0, 0);
      co = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[cb][3], ao(2 * g + 1), co, 0, 0, 0);
    }
  }
}

// odd-half fragment k of a wave: a register, or (KS = 32: the last NFL of them) its slot in LDS
template <int KR>
__device__ __forceinline__ double frag_odd(int k, const double *ao, const double *aoL) { return (k < KR) ? ao[(k < KR) ? k : 0] : aoL[(k - KR) * 64]; }

// exchange with the neighbouring lane (lane ^ 1): DPP quad_perm [1,0,3,2]
__device__ __forceinline__ double swap1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// value of the even lane of each pair / of the odd lane, in both lanes (DPP quad_perm [0,0,2,2] / [1,1,3,3])
__device__ __forceinline__ double bc_even(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0xA0, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0xA0, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double bc_odd(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0xF5, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0xF5, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// The exchange fused with its select: ONE v_cndmask_b32 per dword whose first source carries the DPP quad_perm (the VOP2 DPP form,
// which hipcc does not form from update_dpp + select).  Of the values a, b of a lane (rows 2 rp, 2 rp + 1 of its column)
//   x = the even lane's a in the even lane, the even lane's b in the odd lane   (= odd ? bc_even(b) : a)
//   y = the odd lane's a in the even lane, the odd lane's b in the odd lane     (= odd ? b : bc_odd(a)).
// The VOP2 form reads its mask from VCC: the two lane-parity masks arrive as scalar constants (PAIR_EVEN / PAIR_ODD) and are moved there.
// The rule of bc_even / bc_odd holds: every lane is active while the DPP source is read.  s_mov + s_nop 1 cover the two wait
// states between a VALU write of a register and a DPP read of it, which hipcc does not count across an asm statement -- and for
// that reason a and b must be results of ordinary vector instructions, never of an MFMA (its longer wait is not covered).
constexpr unsigned long long PAIR_EVEN = 0x5555555555555555ull, PAIR_ODD = 0xAAAAAAAAAAAAAAAAull;
__device__ __forceinline__ void xpair(double a, double b, double &x, double &y) {
  const int al = __double2loint(a), ah = __double2hiint(a), bl = __double2loint(b), bh = __double2hiint(b);
  int xl, xh, yl, yh;
  asm("s_mov_b64 vcc, %8\n\t"
      "s_nop 1\n\t"
      "v_cndmask_b32_dpp %0, %6, %4, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_cndmask_b32_dpp %1, %7, %5, vcc quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_mov_b64 vcc, %9\n\t"
      "v_cndmask_b32_dpp %2, %4, %6, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t"
      "v_cndmask_b32_dpp %3, %5, %7, vcc quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf"
      : "=&v"(xl), "=&v"(xh), "=&v"(yl), "=&v"(yh) : "v"(al), "v"(ah), "v"(bl), "v"(bh), "s"(PAIR_EVEN), "s"(PAIR_ODD) : "vcc");
  x = __hiloint2double(xh, xl); y = __hiloint2double(yh, yl);
}

// Descriptor of the window that starts `org` doubles into an array of `len` doubles, formed on the scalar unit: base = a + org as a
// 64-bit address, num_records = the bytes left of the array from there (none when the window starts behind its end, or when
// !valid), at most RSRC_MAX_RECORDS.  An access through it at a per-lane byte offset below RSRC_MAX_RECORDS is in range exactly when
// it lies inside the array; an offset of RSRC_MAX_RECORDS and more is out of range always (the lanes that must not store).
// org and len are wave-uniform and org + the window < 2^32 doubles (the launchers see to it), so arrays of any size below 32 GiB do.
// (The subtraction is written as max - org with one operand hidden from the optimiser: as a saturating difference hipcc computes it
// on the VECTOR unit -- the scalar one has no such instruction -- and the descriptor would sit in vector registers.)
constexpr u32 RSRC_MAX_RECORDS = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_at(const double *a, u32 len, u32 org, bool valid) {
  u32 orgx = org;
  asm("" : "+s"(orgx));
  u32 rem = (len > orgx ? len : orgx) - org;
  rem = rem < RSRC_MAX_RECORDS / 8u ? rem : RSRC_MAX_RECORDS / 8u;
  return __builtin_amdgcn_make_buffer_rsrc((void *)(a + org), 0, valid ? rem * 8u : 0u, 0x00020000);
}

// raw buffer accesses: 32-bit byte offset, the hardware range check is the mask (out-of-range loads return 0, stores are dropped)
__device__ __forceinline__ d2 ld16(__amdgpu_buffer_rsrc_t r, u32 off) { return __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0)); }
__device__ __forceinline__ void st16(__amdgpu_buffer_rsrc_t r, u32 off, d2 v) { __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), r, (int)off, 0, 0); }
__device__ __forceinline__ double ld8(__amdgpu_buffer_rsrc_t r, u32 off) { return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0)); }
__device__ __forceinline__ void st8(__amdgpu_buffer_rsrc_t r, u32 off, double v) { __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, (int)off, 0, 0); }

}  // namespace chebhip
