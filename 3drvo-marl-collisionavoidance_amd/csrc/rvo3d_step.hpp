// rvo3d_step.hpp -- The environment step kernel and its per-drone parts: building gate, observation writers,
// zero fill, rewards, env_kernel<MODE, NW, NFIX, TRAIN, PAD>.
// Part of the gfx950 device code (see rvo3d_device.hpp for the overview).
#pragma once

#include "rvo3d_pairs.hpp"

namespace rvo3d {

// building gate + check_col_with_budilding (rvo_inter.py:99-105, 198-209)
__device__ __forceinline__ bool building_test(const double* const bld, int b, const Drone& S,
                                              double T5) {
  const double bx = bld[4 * b], by = bld[4 * b + 1], bh = bld[4 * b + 2], br = bld[4 * b + 3];
  const double ex = S.x - bx, ey = S.y - by;
  // h > z - 2 and norm <= 5 (gate), z <= h, then dis <= r + br on the few that pass
  if ((bh > S.z - 2) & (norm2sq(ex, ey) <= T5) & (S.z <= bh))
    return __builtin_sqrt(sq(ex) + sq(ey)) <= S.r + br;
  return false;
}
// e: the drone's env (an active lane's: e < P.E).  Per-env sets (rvo3d_set_env_buildings) give the records and the
// cells an element stride per env; with the shared list both strides are 0 and every env reads the one copy.
__device__ __forceinline__ bool building_hit(const Params& P, const Drone& S, int e) {
  const int nb = P.cold().nb;
  if (nb == 0) return false;
  bool hit = false;
  const double* const bld = P.cold().bld + (size_t)e * P.cold().bld_stride;
  const double T5 = P.cold().T5;
  const int gx = P.cold().bgx;
  if (gx > 0) {
    // only the buildings listed for the drone's cell can pass the 5 m gate (the lists are
    // conservative; a drone outside the map collides anyway and NaN passes no test)
    const int gy = P.cold().bgy;
    const double inv = P.cold().bg_inv;
    int ix = (int)__builtin_floor(S.x * inv), iy = (int)__builtin_floor(S.y * inv);
    ix = ix < 0 ? 0 : (ix > gx - 1 ? gx - 1 : ix);
    iy = iy < 0 ? 0 : (iy > gy - 1 ? gy - 1 : iy);
    // the count and the first seven entries in one 16-B load (lists are short: most cells have
    // none or one), the records of two listed buildings per round trip (entry 1 pads the batch:
    // testing a building twice changes nothing); longer lists are walked from memory
    const uint16_t* const cell = P.cold().bgrid + (size_t)e * P.cold().bgrid_stride + (size_t)(ix * gy + iy) * (kBgridK + 1);
    const uint4 c0 = *reinterpret_cast<const uint4*>(cell);
    const int cnt = (int)(c0.x & 0xffffu);
    if (cnt != 0xffff) {
      if (cnt >= 1) {
        const int b0 = (int)(c0.x >> 16), b1 = cnt >= 2 ? (int)(c0.y & 0xffffu) : b0;
        hit |= building_test(bld, b0, S, T5);
        hit |= building_test(bld, b1, S, T5);
      }
      if (cnt >= 3) {
        const int b0 = (int)(c0.y >> 16), b1 = cnt >= 4 ? (int)(c0.z & 0xffffu) : b0;
        hit |= building_test(bld, b0, S, T5);
        hit |= building_test(bld, b1, S, T5);
      }
      for (int k = 5; k <= cnt; ++k) hit |= building_test(bld, (int)cell[k], S, T5);
      return hit;
    }
  }
#pragma unroll 4
  for (int b = 0; b < nb; ++b) hit |= building_test(bld, b, S, T5);
  return hit;
}

// Proprioceptive part of one observation row: np.round of [state, vel, radius,
// priority, des_vel, deviation] (ir_gym.py:208-229 / :353-355), 12 floats.  The last four
// arrive already rounded (`tail`, made by proprio_tail before the final sweep so that the
// fp64 values are dead across it).
struct ProprioTail { float dv0, dv1, dv2, dev; bool bad; };
__device__ __forceinline__ ProprioTail proprio_tail(const double dv[3], double dev) {
  ProprioTail t;
  t.dv0 = round2_f32(dv[0]); t.dv1 = round2_f32(dv[1]); t.dv2 = round2_f32(dv[2]);
  t.dev = round2_f32(dev);
  t.bad = !(finite_d(dv[0]) && finite_d(dv[1]) && finite_d(dv[2]) && finite_d(dev));
  // pin the four floats here: left alone the compiler sinks the final multiply and the conversion
  // below the sweep and keeps (or spills) the four doubles across it instead
  asm volatile("" : "+v"(t.dv0), "+v"(t.dv1), "+v"(t.dv2), "+v"(t.dev));
  return t;
}
__device__ __forceinline__ void write_proprio(const Params& P, int g, const Drone& S,
                                              const ProprioTail& t) {
  float* o = P.obs + (size_t)g * P.W;
  const double v[8] = {S.x, S.y, S.z, S.vx, S.vy, S.vz, S.r, S.prio};
  float f[12];
  bool bad = t.bad;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    f[k] = round2_f32(v[k]);
    bad |= !finite_d(v[k]);
  }
  f[8] = t.dv0; f[9] = t.dv1; f[10] = t.dv2; f[11] = t.dev;
  if ((P.W & 1) == 0) {  // rows are 8-B aligned
    float2* o2 = reinterpret_cast<float2*>(o);
#pragma unroll
    for (int k = 0; k < 6; ++k) o2[k] = make_float2(f[2 * k], f[2 * k + 1]);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = f[k];
  }
  if (bad) atomicOr(P.err, 1u);
}

// 16-B row writer, part 1: the lane's proprioceptive floats go to LDS (float2 [row][6], laid
// over the fp32 image, which is dead by now) together with the start of the row's zero run in
// 8-B units; row_fill_pairs() then writes proprio and zeros of all rows with coalesced 16-B stores.
__device__ __forceinline__ void stage_row(const Params& P, const Lds& L, int tid, int g,
                                          const Drone& S, const ProprioTail& t, int kept) {
  const double v[8] = {S.x, S.y, S.z, S.vx, S.vy, S.vz, S.r, S.prio};
  float f[12];
  bool bad = t.bad;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    f[k] = round2_f32(v[k]);
    bad |= !finite_d(v[k]);
  }
  f[8] = t.dv0; f[9] = t.dv1; f[10] = t.dv2; f[11] = t.dev;
  float4* pro = reinterpret_cast<float4*>(L.w[0]) + 3 * tid;
  pro[0] = make_float4(f[0], f[1], f[2], f[3]);
  pro[1] = make_float4(f[4], f[5], f[6], f[7]);
  pro[2] = make_float4(f[8], f[9], f[10], f[11]);
  L.kept[tid] = ((12 + 9 * kept + 1) & ~1) >> 1;
  // with 8-B units an odd 9*kept leaves one float between the kept rows and the zero run
  if (((9 * kept) & 1) && kept < P.nm) P.obs[(size_t)g * P.W + 12 + 9 * kept] = 0.0f;
  if (bad) atomicOr(P.err, 1u);
}

template <int NW>  // waves of this workgroup (<= NW; T = N rounded up to 64): what the cooperative row writers stride by
__device__ __forceinline__ int waves_of(const Lds& L) { return NW == 1 ? 1 : (L.T >> 6); }

// 16-B row writer, part 2 (W even, obs 16-B aligned).  Two consecutive rows (an even row and
// its successor, counted over the whole obs tensor) are 2 * W * 4 = 16 * q bytes starting on a
// 16-B boundary: q = W / 2 chunks of 16 B.  One wave-instruction stores one row pair: lane c
// owns chunk c of every pair, i.e. two fixed 8-B units (row of the pair, unit inside the row)
// computed once; per pair it looks up the zero runs of its one or two rows and assembles the
// chunk - proprio bytes from LDS, zeros inside a row's zero run, nothing inside the kept VO
// rows (their lane wrote them).  A half outside the workgroup's rows or inside kept rows turns
// the store into an 8-B one.  The waves of the workgroup take the pairs round-robin.
template <int NW>
__device__ __forceinline__ void row_fill_pairs(const Params& P, const Lds& L, int tid, int row0,
                                               int nrows) {
  const int q = P.W >> 1;  // 8-B units per row = 16-B chunks per row pair
  const int ln = tid & 63, wv = tid >> 6;
  const int nwv = waves_of<NW>(L);
  const int pair0 = row0 >> 1;
  const int npairs = ((row0 + nrows + 1) >> 1) - pair0;
  const int rbase = 2 * pair0 - row0;  // local row of the first pair's first row: 0 or -1
  const float2* pro2 = reinterpret_cast<const float2*>(L.w[0]);
  const uint32_t pair_bytes = 8u * (uint32_t)P.W;
  char* const obsb = reinterpret_cast<char*>(P.obs) + (size_t)pair0 * pair_bytes;
  // Row indices -1 and nrows occur at the two ends of the range; the LDS words read for them are
  // valid memory next to the arrays and never used (in0 / in1 are false there).
  for (int cb = 0; cb < q; cb += 64) {  // one trip unless a row has more than 64 chunks
    const int c = cb + ln;
    const bool lane_on = c < q;
    const int h0 = 2 * c, h1 = 2 * c + 1;        // the chunk's halves, as units of the pair
    const int s0 = h0 >= q ? 1 : 0, s1 = h1 >= q ? 1 : 0;
    const int u0 = h0 - (s0 ? q : 0), u1 = h1 - (s1 ? q : 0);
    const bool p0 = u0 < 6, p1 = u1 < 6;         // proprio units
    const int pu0 = p0 ? u0 : 5, pu1 = p1 ? u1 : 5;
    uint32_t off = (uint32_t)wv * pair_bytes + 16u * (uint32_t)c;
    const uint32_t ostep = (uint32_t)nwv * pair_bytes;
    // four pairs per trip: their LDS lookups are issued together (one round trip, not four)
    // and the stores are two flat predicated regions (whole chunk: nearly always; one half:
    // only next to kept rows and at the ends of the range)
    for (int i0 = wv; i0 < npairs; i0 += 4 * nwv) {
      int z0[4], z1[4];
      float2 d0[4], d1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * nwv;  // may run past npairs: reads stay inside the LDS allocation
        const int lr0 = rbase + 2 * i + s0, lr1 = rbase + 2 * i + s1;
        z0[u] = L.kept[lr0]; z1[u] = L.kept[lr1];
        d0[u] = pro2[lr0 * 6 + pu0]; d1[u] = pro2[lr1 * 6 + pu1];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * nwv;
        const int lr0 = rbase + 2 * i + s0, lr1 = rbase + 2 * i + s1;
        const bool live = lane_on & (i < npairs);
        const bool v0 = live & ((unsigned)lr0 < (unsigned)nrows) & (p0 | (u0 >= z0[u]));
        const bool v1 = live & ((unsigned)lr1 < (unsigned)nrows) & (p1 | (u1 >= z1[u]));
        const float2 a = p0 ? d0[u] : make_float2(0.f, 0.f);
        const float2 b = p1 ? d1[u] : make_float2(0.f, 0.f);
        char* const pc = obsb + (off + (uint32_t)u * ostep);
        if (v0 & v1) *reinterpret_cast<float4*>(pc) = make_float4(a.x, a.y, b.x, b.y);
        if (v0 != v1) *reinterpret_cast<float2*>(pc + (v1 ? 8 : 0)) = v1 ? b : a;
      }
      off += 4u * ostep;
    }
  }
}

// ---- two-phase row writer (fused auto-reset step; workgroup rows a multiple of 8, W even, >= 48) --
// The workgroup's rows are then a byte range that starts and ends on 64-B boundaries.  Seen in 64-B
// blocks, a block either holds proprio bytes of some row ("late": 2 of every ~6.4) or only
// VO-region bytes ("early").  The early blocks need no data at all: their zeros are stored BEFORE
// the rows sweep - 69 % of the observation bytes leave while the sweep computes instead of in the
// store burst at the end of the kernel - and a lane whose sweep then keeps VO rows writes them over
// the zeros afterwards (after s_waitcnt vmcnt(0): the zeros of its own wave have landed; workgroups
// of several waves drain before the sweep's second barrier).  The late blocks are written after the
// sweep as 128-B windows, one per row, from the proprio staged in LDS (part 2 below).
// Ordering: `s_waitcnt vmcnt(0)` (+ the workgroup barrier for several waves) makes the early zeros land before a
// kept row is stored over them.  That holds because the waves of a workgroup share one CU's memory pipeline - the
// library is built WITHOUT threadgroup-split mode (no -mtgsplit: hipcc's default), where waves of a workgroup
// could sit on different CUs and a store's completion would not order it against another CU's stores.
// Full workgroups only (the host tabulates the block pattern of a full workgroup, zf_iters > 0:
// W even, 48 <= W <= 128, rows per workgroup a multiple of 8); the last, partial workgroup of a
// launch and other widths take the row-pair writer.
__device__ __forceinline__ bool two_phase_rows(const Params& P, int row0, int nrows, int full_rows) {
  return P.zf16 && P.cold().zf_iters > 0 && nrows == full_rows && (row0 & 7) == 0;
}
// ... of a counted step, which may run on another workgroup shape than the table's (Cold::cnt_two_phase)
__device__ __forceinline__ bool two_phase_rows_counted(const Params& P, int row0, int nrows, int full_rows) {
  return two_phase_rows(P, row0, nrows, full_rows) && P.cold().cnt_two_phase != 0;
}

// part 1: zeros of every 64-B block that holds no proprio byte.  One wave-instruction = 16 blocks
// (1 KB, whole lines).
// With P.prev_cnt (obs holds a consistent pair) a block is stored only where it overlaps an old kept-row
// range [48, 48 + 36 * cnt_old) of its row: every other byte of it is zero already, and the kept rows of
// this step go over it as before.  L.kept holds the old counts (phase 0) until the rows are staged.
template <int NW>
__device__ __forceinline__ void early_zero_blocks(const Params& P, const Lds& L, int tid, int row0,
                                                  int nrows) {
  const uint32_t rb = 4u * (uint32_t)P.W;  // row bytes (a multiple of 8)
  const int ln = tid & 63, wv = tid >> 6;
  const int nwv = waves_of<NW>(L);
  (void)nrows;  // a full workgroup (two_phase_rows)
  char* const base = reinterpret_cast<char*>(P.obs) + (size_t)row0 * rb;
  const uint32_t blk = (uint32_t)wv * 16u + ((uint32_t)ln >> 2);
  typedef float v4f __attribute__((ext_vector_type(4)));
  // which trips store is a property of the thread quad, tabulated by the host (rvo3d_create): no
  // per-trip offset arithmetic.  Ordinary stores, like the windows of part 2.
  const int iters = P.cold().zf_iters;
  uint32_t m = P.cold().zmask[tid >> 2];
  if (P.prev_cnt) {
    // the common case - no row of the workgroup had a kept row - stores nothing at all (L.kept: the
    // workgroup's rows are [0, T) for one wave; several waves raised L.any_old in phase 0)
    const bool any = NW == 1 ? __ballot(L.kept[tid] != 0) != 0
                             : __builtin_amdgcn_readfirstlane(*L.any_old) != 0;
    if (!any) return;
    // trip i meets the block at byte o = blk * 64 + i * 1024 * nwv of the workgroup's rows, inside the VO
    // region of row o / rb.  With zf_iters <= 32 and >= 8 rows, o < 2^18 (exact in fp32) and rb <= 2^15: the
    // quotient (< 512) is >= 48 / rb >= 2^-10 away from an integer (an early block starts >= 48 B into a row
    // and ends inside it), the fp32 product is off by < 2^-14 and truncates to the row exactly.
    const float inv_rb = 1.0f / (float)rb;
    const uint32_t st = 1024u * (uint32_t)nwv;
    uint32_t keep = 0;
    for (int i = 0; i < iters; ++i)
      if ((m >> i) & 1u) {
        const uint32_t o = blk * 64u + (uint32_t)i * st;
        const uint32_t r = (uint32_t)((float)o * inv_rb);
        if (o - r * rb < 48u + 36u * (uint32_t)L.kept[r]) keep |= 1u << i;
      }
    m = keep;
  }
  char* p = base + (size_t)blk * 64u + 16u * ((uint32_t)ln & 3u);
  const size_t step = (size_t)1024 * (size_t)nwv;
  // four trips per loop pass (bits beyond the last trip are 0: nothing is stored for them)
  for (int i = 0; i < iters; i += 4, p += 4 * step, m >>= 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if ((m >> u) & 1u) {
        *reinterpret_cast<v4f*>(p + u * step) = (v4f){0.f, 0.f, 0.f, 0.f};
      }
  }
}

// part 2: per row the 128-B window that starts at the 64-B block holding the row's first byte: the
// tail of the previous row's VO region (s bytes), the 48 proprio bytes, the head of this row's VO
// region.  Eight rows per wave-instruction, lane = (row, 16-B chunk); 8-B halves as in
// row_fill_pairs: proprio from LDS, zeros inside a zero run, nothing inside kept rows.
template <int NW>
__device__ __forceinline__ void late_row_windows(const Params& P, const Lds& L, int tid, int row0,
                                                 int nrows) {
  const uint32_t rb = 4u * (uint32_t)P.W, q = rb >> 3;  // row bytes, 8-B units per row
  const int ln = tid & 63, wv = tid >> 6;
  const int nwv = waves_of<NW>(L);
  const float2* pro2 = reinterpret_cast<const float2*>(L.w[0]);
  char* const base = reinterpret_cast<char*>(P.obs) + (size_t)row0 * rb;
  const int ch = ln & 7;
  const int r0 = wv * 8 + (ln >> 3);
  // A trip advances every lane by 8 * nwv rows = a multiple of 64 B (W is even): where the lane's
  // chunk sits relative to its row - which of its two 8-B units belong to the previous row's tail,
  // which are proprio, which unit of the row they are - is the same in every trip.  Only the row
  // itself (its kept count, its proprio floats) changes.
  const uint32_t rs0 = rb * (uint32_t)r0;      // row start of the first trip, relative to the workgroup's range
  const uint32_t s8 = (rs0 & 63u) >> 3;        // units of the window that belong to row r - 1
  const uint32_t ua = 2u * (uint32_t)ch, ub = ua + 1u;
  const bool pa = ua < s8, pb = ub < s8;       // in the previous row's tail (never in row 0: s8 = 0 there)
  const uint32_t uia = pa ? q - s8 + ua : ua - s8, uib = pb ? q - s8 + ub : ub - s8;
  const bool proa = uia < 6u, prob = uib < 6u;
  const int pia = (int)(proa ? uia : 5u), pib = (int)(prob ? uib : 5u);
  const int da_row = pa ? 1 : 0, db_row = pb ? 1 : 0;
  char* pc = base + (rs0 & ~63u) + 16u * (uint32_t)ch;
  const size_t step = (size_t)8 * (size_t)nwv * rb;
  for (int r = r0; r < nrows; r += 8 * nwv, pc += step) {
    const int ra = r - da_row, rbw = r - db_row;
    const int za = L.kept[ra], zb = L.kept[rbw];
    const float2 da = pro2[ra * 6 + pia], db = pro2[rbw * 6 + pib];
    const bool va = proa | (uia >= (uint32_t)za), vb = prob | (uib >= (uint32_t)zb);
    const float2 a = proa ? da : make_float2(0.f, 0.f), b = prob ? db : make_float2(0.f, 0.f);
    if (va & vb) *reinterpret_cast<float4*>(pc) = make_float4(a.x, a.y, b.x, b.y);
    if (va != vb) *reinterpret_cast<float2*>(pc + (vb ? 8 : 0)) = vb ? b : a;
  }
}

// The kept VO rows of one observation row (np.round(., 2) of [PAA, rel, alpha, min_dis,
// iet] per row, ascending urgency) and its vo_count.  The zeros behind them are the row
// writers' business (row_fill_pairs / the two-phase writer / zero_fill).
__device__ __forceinline__ void write_vo_rows(const Params& P, const Lds& L, int tid, int lbase,
                                              int g, const Drone& S, int kept) {
  float* o = P.obs + (size_t)g * P.W;
  bool bad = false;
  for (int s = 0; s < kept; ++s) {
    const uint32_t pk = P.row_pk(s)[g];
    const int j = (int)(pk & 0xffffu);
    const Drone O = lds_drone(L, lbase + j);
    const double pr = (S.prio == O.prio) ? 0.5 : S.prio / (S.prio + O.prio);
    double row[9];
    row[0] = pr * (2 * S.x + (S.vx + O.vx));  // get_PAA, vel_obs3D.py:19-32
    row[1] = pr * (2 * S.y + (S.vy + O.vy));
    row[2] = pr * (2 * S.z + (S.vz + O.vz));
    row[3] = O.x - S.x; row[4] = O.y - S.y; row[5] = O.z - S.z;
    row[6] = (double)(pk >> 16) / 100.0;
    row[7] = pair_md(S, O);
    row[8] = P.row_iet(s)[g];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      bad |= !finite_d(row[k]);
      o[12 + 9 * s + k] = round2_f32(row[k]);
    }
  }
  P.vo_count[g] = kept;
  if (bad) atomicOr(P.err, 1u);
}

// Generic row writer (W odd, or obs not 16-B aligned; the 16-B path is stage_row + row_fill_pairs).
// The zero run behind the kept rows of one observation row: with 8-B zero-fill units an odd
// 9 * kept leaves one float for this lane.
__device__ __forceinline__ void publish_zero_run(const Params& P, int g, int kept) {
  if ((P.W & 1) == 0 && ((9 * kept) & 1) && kept < P.nm) P.obs[(size_t)g * P.W + 12 + 9 * kept] = 0.0f;
}

// Counted kernels: the live drones of env e (rvo3d_set_drone_counts), read like the rest of Cold through the constant
// address space - a scalar load where the env is the workgroup's.
__device__ __forceinline__ int live_count(const Params& P, int e) {
  return ((const __attribute__((address_space(4))) int32_t*)P.cold().counts)[e];
}
// Counted kernels: the row of a ghost inside the layout - all zeros, vo_count 0 - through the same row writers: zero
// proprio staged like stage_row's with the zero run right behind it (row_fill_pairs / late_row_windows; the early
// blocks are zeros anyway), or the twelve floats stored here with no kept row (zero_fill).
__device__ __forceinline__ void ghost_row(const Params& P, const Lds& L, int lrow, int g) {
  P.vo_count[g] = 0;
  if (P.zf16) {
    float4* pro = reinterpret_cast<float4*>(L.w[0]) + 3 * lrow;
    pro[0] = pro[1] = pro[2] = make_float4(0.f, 0.f, 0.f, 0.f);
    L.kept[lrow] = 6;
  } else {
    float* o = P.obs + (size_t)g * P.W;
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = 0.0f;
    L.kept[lrow] = 0;
  }
}
// ... and its other outputs of a step
__device__ __forceinline__ void ghost_outputs(const Params& P, int g, bool lite) {
  P.reward[g] = 0.0f;
  if (P.reward64) P.reward64[g] = 0.0;
  P.done[g] = 0; P.info[g] = 0; P.finish[g] = 0;
  if (lite && P.reset_mask) P.reset_mask[g] = 0;
}

// Cooperative, coalesced zero padding of the VO region of every row of this
// workgroup: rows [row0, row0 + nrows) are contiguous in memory; L.kept holds
// the kept count per row.  Unit = float2 when W is even (rows 8-B aligned),
// float otherwise.  q < T * per_row (validated by rvo3d_create for the 32-bit magic).
__device__ __forceinline__ void zero_fill(const Params& P, const Lds& L, int tid, int row0,
                                          int nrows) {
  const uint32_t per_row = P.cold().zf_div;
  if (per_row == 0) return;
  const uint32_t total = (uint32_t)nrows * per_row;
  float* base = P.obs + (size_t)row0 * P.W + 12;
  if ((P.W & 1) == 0) {
    for (uint32_t q = tid; q < total; q += L.T) {
      const uint32_t row = (uint32_t)(((uint64_t)q * P.cold().zf_magic) >> 32);
      const uint32_t c = q - row * per_row;       // float2 index inside the VO region
      const uint32_t first = (9u * (uint32_t)L.kept[row] + 1u) >> 1;  // first all-zero unit
      if (c >= first)
        *reinterpret_cast<float2*>(base + (size_t)row * P.W + 2 * c) = make_float2(0.f, 0.f);
    }
  } else {
    for (uint32_t q = tid; q < total; q += L.T) {
      const uint32_t row = (uint32_t)(((uint64_t)q * P.cold().zf_magic) >> 32);
      const uint32_t c = q - row * per_row;
      if (c >= 9u * (uint32_t)L.kept[row]) base[(size_t)row * P.W + c] = 0.0f;
    }
  }
}

__device__ __forceinline__ void load_wp(const Params& P, int g, int k, double out[3]) {
  out[0] = P.wp(k, 0)[g];
  out[1] = P.wp(k, 1)[g];
  out[2] = P.wp(k, 2)[g];
}

__device__ __forceinline__ void load3(double* const a0, double* const a1, double* const a2, int g,
                                      double out[3]) {
  out[0] = a0[g]; out[1] = a1[g]; out[2] = a2[g];
}
__device__ __forceinline__ void store3(double* const a0, double* const a1, double* const a2, int g,
                                       const double v[3]) {
  a0[g] = v[0]; a1[g] = v[1]; a2[g] = v[2];
}

// ir_gym.rvo_reward_cal (ir_gym.py:64-133), the part that does not depend on the sweep:
// angle_punish + vel_penalty.  The sweep's safety term is added afterwards in the
// reference's order, (punish + vel_penalty) + safety: rvo_reward_k().
__device__ __forceinline__ double rvo_reward_pre(const double dv[3], const double a[3]) {
  // des_vel is already a 3-decimal value: np.round(., 3) again is the identity
  const double d0 = dv[0], d1 = dv[1], d2 = dv[2];
  const double vel_penalty = 0.2 * norm3b(a[0], a[1], a[2]) / norm3b(d0, d1, d2);
  const double eps = 1e-8;
  const double magA = __builtin_sqrt(sq(d0) + sq(d1) + sq(d2) + eps);
  const double magB = __builtin_sqrt(sq(a[0]) + sq(a[1]) + sq(a[2]) + eps);
  const double dotp = d0 * a[0] + d1 * a[1] + d2 * a[2];
  double c = dotp / (magA * magB);  // magA, magB >= 1e-4: the `< 1e-6` branch is dead
  c = c < -1.0 + eps ? -1.0 + eps : (c > 1.0 - eps ? 1.0 - eps : c);
  // angle bins (ir_gym.py:91-100) on ang = acos(c): compare c with the cosines of
  // the bin edges; acos itself only when c is within 1e-12 of an edge.
  const double C18 = 0.984807753012208, C6 = 0.8660254037844387, C3 = 0.5000000000000001,
               C2 = 6.123233995736766e-17;
  double punish;
  if (c == 0.0) punish = -4;  // acos(0) == pi/2 exactly: not < pi/2
  else if (__builtin_fabs(c - C18) > 1e-12 && __builtin_fabs(c - C6) > 1e-12 &&
           __builtin_fabs(c - C3) > 1e-12 && __builtin_fabs(c - C2) > 1e-12) {
    punish = c > C18 ? 3 : (c > C6 ? 1 : (c > C3 ? 0.5 : (c > C2 ? 0 : -4)));
    if (c != c) punish = -4;
  } else {
    const double ang = acos(c);
    if (ang < kPi / 18) punish = 3;
    else if (ang < kPi / 6) punish = 1;
    else if (ang < kPi / 3) punish = 0.5;
    else if (ang < kPi / 2) punish = 0;
    else punish = -4;
  }
  return punish + vel_penalty;
}
// Returns the integer k with np.round(total, 3) == k / 1000 (or inf / nan, survey Q9).
__device__ __forceinline__ double rvo_reward_k(double pre, bool flag, double tmin) {
  double safety = 0;
  if (flag) {
    double urgency = 0;
    if (tmin < 2) urgency = -8.0 * exp(-tmin / 0.5);
    safety = -2.5 + urgency;
  }
  return __builtin_rint((pre + safety) * 1000.0);
}

// ir_gym.mov_reward (ir_gym.py:256-311); returns k with round(., 3) == k / 1000
__device__ __forceinline__ double mov_reward_k(const Params& P, bool collision, bool arrive_r,
                                               int waypoint_num, int n_points_m1, bool dest_r,
                                               double dev, bool len_flag, double exlen) {
  if (collision) return -50000.0;  // -50
  double reward = 0;
  if (arrive_r) reward += 3.0 * P.cold().pow95[n_points_m1 - waypoint_num];
  if (dest_r) reward += 20.0;
  const double d = dev * 10;
  const double dev_pen = -1.5 * (2 / (1 + exp(-(d - 5) / 0.3)));
  double ex_pen = 0;
  if (len_flag) {
    ex_pen = -0.3 * log(exlen + 1 + 1e-6);
    if (ex_pen < -6 || ex_pen != ex_pen) ex_pen = -6;
  }
  return __builtin_rint((reward + dev_pen + ex_pen) * 1000.0);
}

// mdin.py:28 adds two np.round(., 3) values in fp64; k / 1000 is formed exactly (k_over_1000)
// so the sum, cancellation included, is the reference's double (stored as float32, and as it is
// into the optional float64 output).

enum Mode { kObserve = 0, kStep = 1, kStepAutoReset = 2 };

// The old count of a row (consistent obs / vo_count pair, early_zero_blocks) as it is filed in L.kept: clamped to nm
// (more only stores more; the clamp bounds what early_zero_blocks adds to a row's kept range).  The count itself is
// requested raw, together with the loads around it: clamping at the load made it a round trip of its own.
__device__ __forceinline__ int clamp_kept(const Params& P, uint32_t c) {
  return (int)(c < (uint32_t)P.nm ? c : (uint32_t)P.nm);
}

// 128 VGPRs = 4 waves per SIMD.  One-wave workgroups (N <= 64): the 4096 waves of 64 x 4096 are
// all resident at once.  N <= 256 (one env per workgroup of 2 or 4 waves): the fourth wave per
// SIMD is what lets 4 workgroups of 256 drones (40 KB of LDS each) share a CU, and shortens the
// tail for the shapes in between (100 drones x 2048 envs: 67.8 -> 55.6 us) - at the price of
// some spills above 128 drones.  N > 256 is LDS-bound to one or two workgroups per CU: 3 per SIMD.
#ifndef RVO3D_WAVES_ATTR
#define RVO3D_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(NW <= 4 ? 4 : 3)))
#endif

// The whole environment step, one launch.
// NFIX > 0: the instantiation for exactly NFIX drones per env (16, 32, 64: 64 / NFIX envs per
// one-wave workgroup; 128, 256: one env per workgroup of NFIX threads): N, the envs per
// workgroup and the workgroup size are compile-time constants, so the LDS layout and the
// index arithmetic of the sweeps fold.  NFIX = 0: any N <= 64 * NW.
// TRAIN = rvo_inter.env_train (rvo_inter.py:14), a compile-time constant of the instantiation.
// PAD: the compile-time kernel takes any N <= NFIX (ghost lanes, see below).  Multi-wave NFIX kernels are always
// padded; the one-wave ones exist in both flavours (the exact one keeps N a compile-time constant everywhere).
// CNT: the live drones are a number per env (rvo3d_set_drone_counts; P.cold().counts) instead of the launch's Pin.N,
// which stays the stride of every [E][N] layout.  The rows d >= counts[e] of an env are ghosts: parked at infinity like
// the lanes beyond the layout, and - being rows of the outputs - written as zeros (ghost_row, ghost_outputs).
// env_kernel (CNT = false, what a handle without counts runs) and env_kernel_counted share ONE body, the text of
// rvo3d_step_body.hpp, included inside the braces of each: the plain kernels then compile to the machine code they had
// before the counted ones existed, which a shared __device__ function does not give.  That file is a fragment, not a
// header: it must never be included anywhere but in the two kernels below.
// The two-phase test of the body (for CNT = false the old call, token for token):
#define RVO3D_TWO_PHASE_ROWS \
  (CNT ? two_phase_rows_counted(P, row0, nrows, full_rows) : two_phase_rows(P, row0, nrows, full_rows))
template <int MODE, int NW, int NFIX = 0, bool TRAIN = true, bool PAD = (NFIX != 0 && NW > 1)>
__global__ void __launch_bounds__(64 * NW) RVO3D_WAVES_ATTR env_kernel(const Params Pin) {
  constexpr bool CNT = false;  // what a handle without drone counts runs: the symbols and the code of every build before them
#include "rvo3d_step_body.hpp"
}
// What a handle with drone counts runs: always a padded compile-time ring (host: pick_counted_kernel).
template <int MODE, int NW, int NFIX, bool TRAIN>
__global__ void __launch_bounds__(64 * NW) RVO3D_WAVES_ATTR env_kernel_counted(const Params Pin) {
  constexpr bool PAD = true, CNT = true;
#include "rvo3d_step_body.hpp"
}

#undef RVO3D_TWO_PHASE_ROWS

}  // namespace rvo3d
