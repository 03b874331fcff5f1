// wk_env_side.h -- the side-split mapping of the env-step (k_env_side): a lane pair or a lane
// quad per walker, the policy on the matrix cores.  Three translation units instantiate it, each
// with its own switches and flags: wk_env_pair.hip, wk_env_quad.hip and, for both mappings on the
// rough floor, wk_env_side_rough.hip.
#pragma once
#include "wk_env_pairs.h"
#include "wk_mfma_layout.h"
#include "wk_sample.h"

namespace wk {

// ---------------- side-split mapping: a lane pair per walker (L = 2) ----------------
// Lane `side` of the pair (0 = left leg, 1 = right leg) owns that leg's two segments; the
// torso is held replicated by both.  Inside StepObjects (Environment.cs:130-142) the
// RigidBody.Step calls run in list order LLL, LLU, BODY, RLL, RLU and every candidate
// pair is either inside one leg or against the static floor (Walker.cs:212-234), so the
// left and right collision chains touch disjoint bodies: both run at once, one per lane,
// and the torso's own step + floor pair runs replicated (bit-identical in both lanes).
// Joints 0 and 1 (Walker.cs:182-187) both move the torso, so they run one lane at a time
// with the torso copied across the pair after each; joints 2 and 3 run at once.  Every
// per-body operation is the same op sequence as the one-lane mapping, so trajectories
// stay bit-identical to the oracle.
struct SideState {
  Poly<6> lo, up;  // this side's lower / upper leg segment
  Poly<5> body;
  Dyn dlo, dup, dbody;
  bool clo, cup, cbody;
  float tq_up, tq_lo;  // joint torques [side] (body-upper) and [2 + side] (upper-lower)
  float posx, posy, prevx, prevy;
  int steps, episodes;
  bool post, terminal;
};

// the legs' 24 vertex coordinates (NR = 6 records; NR = 4: the first 16 of them) to / from a
// lane's float4 column (stride FS): the rough floor's own stash, see k_env_side.  (The flat
// floor's kernel parks them in its face column's planes: park_legs_planes, wk_device.h.)
template <int FS, int NR = 6>
DEV void park_legs(const SideState& s, float4* r) {
  r[0 * FS] = make_float4(s.lo.x[0], s.lo.x[1], s.lo.x[2], s.lo.x[3]);
  r[1 * FS] = make_float4(s.lo.x[4], s.lo.x[5], s.lo.y[0], s.lo.y[1]);
  r[2 * FS] = make_float4(s.lo.y[2], s.lo.y[3], s.lo.y[4], s.lo.y[5]);
  r[3 * FS] = make_float4(s.up.x[0], s.up.x[1], s.up.x[2], s.up.x[3]);
  if constexpr (NR == 6) {
    r[4 * FS] = make_float4(s.up.x[4], s.up.x[5], s.up.y[0], s.up.y[1]);
    r[5 * FS] = make_float4(s.up.y[2], s.up.y[3], s.up.y[4], s.up.y[5]);
  }
}
template <int FS, int NR = 6>
DEV void unpark_legs(SideState& s, const float4* r) {
  float4 a = r[0 * FS], b = r[1 * FS], c = r[2 * FS];
  s.lo.x[0] = a.x; s.lo.x[1] = a.y; s.lo.x[2] = a.z; s.lo.x[3] = a.w;
  s.lo.x[4] = b.x; s.lo.x[5] = b.y; s.lo.y[0] = b.z; s.lo.y[1] = b.w;
  s.lo.y[2] = c.x; s.lo.y[3] = c.y; s.lo.y[4] = c.z; s.lo.y[5] = c.w;
  a = r[3 * FS];
  s.up.x[0] = a.x; s.up.x[1] = a.y; s.up.x[2] = a.z; s.up.x[3] = a.w;
  if constexpr (NR == 6) {
    b = r[4 * FS]; c = r[5 * FS];
    s.up.x[4] = b.x; s.up.x[5] = b.y; s.up.y[0] = b.z; s.up.y[1] = b.w;
    s.up.y[2] = c.x; s.up.y[3] = c.y; s.up.y[4] = c.z; s.up.y[5] = c.w;
  }
}

template <int CTRL>
DEV float dppc(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
DEV float pswap(float v) { return dppc<0xB1>(v); }  // quad_perm [1,0,3,2]: the partner lane

// copy the torso from the even (CTRL = quad_perm [0,0,2,2]) or odd ([1,1,3,3]) lane
template <int CTRL>
DEV void bcast_torso(Poly<5>& b, Dyn& d) {
#pragma unroll
  for (int i = 0; i < 5; i++) { b.x[i] = dppc<CTRL>(b.x[i]); b.y[i] = dppc<CTRL>(b.y[i]); }
  b.cx = dppc<CTRL>(b.cx); b.cy = dppc<CTRL>(b.cy);
  d.vx = dppc<CTRL>(d.vx); d.vy = dppc<CTRL>(d.vy); d.w = dppc<CTRL>(d.w);
}

DEV void load_side(SideState& s, const float* __restrict__ st, int e, int side) {
  const int blo = side ? RLL : LLL, bup = side ? RLU : LLU;
  load_poly(s.lo, st, blo, e, 0);
  load_poly(s.up, st, bup, e, 0);
  load_poly(s.body, st, BODY, e, 0);
  load_dyn(s.dlo, s.clo, st, blo, e, 0);
  load_dyn(s.dup, s.cup, st, bup, e, 0);
  load_dyn(s.dbody, s.cbody, st, BODY, e, 0);
  const float* r = st + (size_t)e * NSTATE;
  s.tq_up = r[S_TORQUE + side];
  s.tq_lo = r[S_TORQUE + 2 + side];
  s.posx = r[S_POS]; s.posy = r[S_POS + 1];
  s.prevx = r[S_PREV]; s.prevy = r[S_PREV + 1];
  s.steps = (int)r[S_STEPS];
  s.post = r[S_POSTRESET] != 0.0f;
  s.terminal = r[S_TERMINAL] != 0.0f;
  s.episodes = (int)r[S_EPISODES];
}

DEV void store_side(const SideState& s, float* __restrict__ st, int e, int side) {
  store_body(s.lo, s.dlo, s.clo, st, side ? RLL : LLL, e, 0);
  store_body(s.up, s.dup, s.cup, st, side ? RLU : LLU, e, 0);
  float* r = st + (size_t)e * NSTATE;
  r[S_TORQUE + side] = s.tq_up;
  r[S_TORQUE + 2 + side] = s.tq_lo;
  if (side == 0) {
    store_body(s.body, s.dbody, s.cbody, st, BODY, e, 0);
    r[S_POS] = s.posx; r[S_POS + 1] = s.posy;
    r[S_PREV] = s.prevx; r[S_PREV + 1] = s.prevy;
    r[S_STEPS] = (float)s.steps;
    r[S_POSTRESET] = s.post ? 1.0f : 0.0f;
    r[S_TERMINAL] = s.terminal ? 1.0f : 0.0f;
    r[S_EPISODES] = (float)s.episodes;
  }
}

// Walker.CreateCreature / Reset (both legs are the same two poles) -- cf. make_template
DEV void make_template_side(SideState& s, float dx) {
  float px = 125.0f + dx, py = 800.0f;
  s.body.x[0] = px + 20; s.body.y[0] = py + 20;
  s.body.x[1] = px;      s.body.y[1] = py + 20;
  s.body.x[2] = px - 20; s.body.y[2] = py + 20;
  s.body.x[3] = px - 20; s.body.y[3] = py - 20;
  s.body.x[4] = px + 20; s.body.y[4] = py - 20;
  find_centroid(s.body);
  make_pole(s.up, px + 0.0f, py + 30.0f);
  make_pole(s.lo, px + 0.0f, py + 60.0f);
  zero_dyn(s.dlo); zero_dyn(s.dup); zero_dyn(s.dbody);
  s.clo = s.cup = s.cbody = false;
  s.tq_up = 0.0f; s.tq_lo = 0.0f;
  s.steps = 0;
  s.terminal = false;
  s.prevx = px; s.prevy = py;
  s.posx = s.body.cx; s.posy = s.body.cy;
}

// Walker.GetState (Walker.cs:132-152) assembled from both lanes of the pair
DEV void get_obs_side(const SideState& s, int side, float o[12]) {
  const float ux = s.up.x[2], uy = s.up.y[2], tlo = s.dlo.th, tup = s.dup.th;
  const float oux = pswap(ux), ouy = pswap(uy), otlo = pswap(tlo), otup = pswap(tup);
  const bool left = side == 0;
  o[0] = s.body.x[1] / 900.0f;
  o[1] = s.body.y[1] / 500.0f;
  o[2] = (left ? ux : oux) / 900.0f;
  o[3] = (left ? uy : ouy) / 500.0f;
  o[4] = (left ? oux : ux) / 900.0f;
  o[5] = (left ? ouy : uy) / 500.0f;
  o[6] = s.dbody.vx / 60.0f;
  o[7] = s.dbody.vy / 60.0f;
  o[8] = left ? tlo : otlo;
  o[9] = left ? tup : otup;
  o[10] = left ? otlo : tlo;
  o[11] = left ? otup : tup;
}

// The torso's RigidBody.Step (RigidBody.cs:54-96), replicated in every lane of the walker (traced
// by the left lane): integrate, then its only candidate, the floor.  It reads and writes the torso
// alone (its leg pairs are associated bodies, Walker.cs:202-209), and no leg step reads the torso,
// so it commutes with the legs' steps that precede it in the list [LLL, LLU, Body, RLL, RLU]:
// substep_side runs it right after the joints, in the lower leg's integrate's basic
// block, where the two independent integrate chains interleave (bit-identical either way; round 5,
// within noise).
template <bool TRACE, bool ROUGH, int TS>
DEV void torso_step(SideState& s, const Mat& mb, float dt, float adx, float ady, PairTraceDev* tr,
                    int side, RegionProf* rp, const float* ter) {
  integrate(s.body, s.dbody, dt, adx, ady);
  rp_mark(rp, RP_INTEG, s.body.x[0], s.body.y[3], s.dbody.th);
  if constexpr (ROUGH) {
    floor_pairs<5, TRACE, 1, true, TS>(s.body, s.dbody, mb, s.cbody, side == 0 ? tr : nullptr, 4, 0, ter);
  } else {
    Poly<4> fl;
    floor_poly(fl);
    Dyn dfl;
    zero_dyn(dfl);
    const Mat mf{0.0f, 0.0f, 0.3f, 1.0f};
    resolve_pair<5, 4, true, TRACE, 1>(s.body, s.dbody, mb, fl, dfl, mf, s.cbody,
                                       side == 0 ? tr : nullptr, 4, 0, rp);
  }
}

// ROUGH: the floor candidates are CreateRoughFloor's 10 segments (floor_pairs, general SAT /
// contacts, replicated in both halves of the quad mapping; ter: this walker's terrain column in
// LDS with stride TS); the leg-leg pairs keep their split
template <bool TRACE, int Q, bool ROUGH = false, int TS = 1, int FS = 0>
DEV void substep_side(SideState& s, const Mat& mp, const Mat& mb, float dt, float adx, float ady,
                      PairTraceDev* tr, int side, int half, RegionProf* rp, const float* ter = nullptr,
                      float* frec = nullptr) {
  rp_mark(rp, RP_OTHER);
  Poly<4> fl;
  floor_poly(fl);
  Dyn dfl;
  zero_dyn(dfl);
  const Mat mf{0.0f, 0.0f, 0.3f, 1.0f};
  // joints [bodyJointLeft, bodyJointRight, leftJoint, rightJoint] (Walker.cs:182-187)
  if (side == 0) joint_step<5, 6, 1, 4, TRACE>(s.body, s.dbody, mb, s.up, s.dup, mp, tr, 0);
  bcast_torso<0xA0>(s.body, s.dbody);
  if (side == 1) joint_step<5, 6, 1, 4, TRACE>(s.body, s.dbody, mb, s.up, s.dup, mp, tr, 1);
  bcast_torso<0xF5>(s.body, s.dbody);
  joint_step<6, 6, 2, 3, TRACE>(s.up, s.dup, mp, s.lo, s.dlo, mp, tr, 2 + side);
  rp_mark(rp, RP_JOINT, s.dup.w, s.dlo.w, s.up.x[0], s.lo.x[0], s.dbody.w, s.body.x[0]);
  // this leg's RigidBody.Step calls (lower then upper); a segment's two candidates run
  // floor-first after a reset, floor-last in episode 0: three slots keep a wave with
  // both kinds of walkers at three pair evaluations instead of four
  const int pb = side ? 5 : 0;
  torso_step<TRACE, ROUGH, TS>(s, mb, dt, adx, ady, tr, side, rp, ter);
  integrate(s.lo, s.dlo, dt, adx, ady);
  rp_mark(rp, RP_INTEG, s.lo.x[0], s.lo.y[3], s.lo.x[5], s.dlo.th);
#pragma unroll
  for (int q = 0; q < 3; q++) {  // [floor if post], other segment, [floor if episode 0]
    if (q == 1) resolve_pair<6, 6, false, TRACE, 1, false, Q, FS>(s.lo, s.dlo, mp, s.up, s.dup, mp, s.clo, tr, pb + 0, half, rp, nullptr, frec);
    else if ((q == 0) == s.post) {
      if constexpr (ROUGH) floor_pairs<6, TRACE, 1, true, TS>(s.lo, s.dlo, mp, s.clo, tr, pb + 1, 0, ter);
      else resolve_pair<6, 4, true, TRACE, 1, false, Q, FS>(s.lo, s.dlo, mp, fl, dfl, mf, s.clo, tr, pb + 1, half, rp, nullptr, frec);
    }
    rp_mark(rp, RP_OTHER);
  }
  integrate(s.up, s.dup, dt, adx, ady);
  rp_mark(rp, RP_INTEG, s.up.x[0], s.up.y[3], s.up.x[5], s.dup.th);
#pragma unroll
  for (int q = 0; q < 3; q++) {
    if (q == 1) resolve_pair<6, 6, false, TRACE, 1, false, Q, FS>(s.up, s.dup, mp, s.lo, s.dlo, mp, s.cup, tr, pb + 2, half, rp, nullptr, frec);
    else if ((q == 0) == s.post) {
      if constexpr (ROUGH) floor_pairs<6, TRACE, 1, true, TS>(s.up, s.dup, mp, s.cup, tr, pb + 3, 0, ter);
      else resolve_pair<6, 4, true, TRACE, 1, false, Q, FS>(s.up, s.dup, mp, fl, dfl, mf, s.cup, tr, pb + 3, half, rp, nullptr, frec);
    }
    rp_mark(rp, RP_OTHER);
  }
  rp_mark(rp, RP_OTHER);
}

DEV bool side_finite(const SideState& s) {  // this side's legs and the torso (see state_finite)
  const float acc = nonfinite_acc(s.lo, s.dlo) + nonfinite_acc(s.up, s.dup) + nonfinite_acc(s.body, s.dbody);
  return acc == 0.0f;
}

// PPOAgent.SampleActions / GetValueEstimate forward passes (NeuralNetwork.FeedForward,
// DenseLayer.cs:82-98) for the 32 walkers of a wave on the matrix cores, with the layouts
// of wk_ppo_mfma.hip: observations staged through LDS into v_mfma_f32_16x16x4_f32 B
// operands (walkers on n, two 16-walker tiles), W1 / W2 A operands streamed from the
// operand-order image (wk_mfma_layout.h, L2-resident), layer 2 chained on layer 1's D
// registers, and the 64-long output rows (actor W3, critic Wc2) on the VALU summed over
// the four lane groups.  fp32 throughout; only the association of the k-sums differs
// from the sequential reference (parity tests: rtol 1e-5).
typedef float pf4 __attribute__((ext_vector_type(4)));
// an opaque copy of a lane value: the address arithmetic built on it is redone where it is used
// instead of being strength-reduced into per-lane 64-bit pointers that live across a loop
DEV uint32_t lane_opaque(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}
// the trajectory rows as plain stores.  Written bytes per rollout launch at 65,536 walkers
// (rollouts only, profiles/r05_write_probe.txt): non-temporal 439 MiB, plain 403 MiB against 384
// MiB algorithmic (385 MiB with the identity lane order): a walker the lane order moved into
// another wave writes into lines that wave fills, and plain stores let the L2 merge those parts
// before the line is written back; the one-byte done rows likewise (their 32 bytes per wave share
// a 128-byte line with three other waves).  Time unchanged.
template <typename T>
DEV void st_row(T v, T* p) { *p = v; }
DEV void st_row4(float* p, float a, float b, float c, float d) {
  const pf4 v = {a, b, c, d};
  st_row(v, (pf4*)p);
}
DEV pf4 pmfma(float a, float b, pf4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
DEV float plrelu(float z) { return z < 0.0f ? 0.2f * z : z; }  // == Math.Max(0.2 z, z), see mf_lrelu

// Q = 2 (quad mapping): 16 walkers per wave, one N tile
template <int Q>
DEV void policy_mfma(const float* __restrict__ Wz, const float obs[12], bool writer,
                     float* __restrict__ pl, float z3[4], float& value, int tx) {
  using namespace mf;
  constexpr int NT = 2 / Q;  // 16-walker tiles per wave
  const int lane = tx & 63, n = lane & 15, g = lane >> 4, wl = lane >> (Q == 2 ? 2 : 1);
  float* tile = pl;          // [32 walkers][16]: 12 observations
  float* outs = pl + 512;    // [32 walkers][8]: z3[0..3], critic output (disjoint from tile)
  if (writer) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const pf4 v = {obs[4 * q], obs[4 * q + 1], obs[4 * q + 2], obs[4 * q + 3]};
      *(pf4*)(tile + wl * 16 + 4 * q) = v;
    }
  }
  wave_lds_sync();
  // one 16-walker tile at a time (not unrolled): a tile's layer-1 activations (16 VGPRs) are
  // the only large live set, so the physics state around the call stays in registers
  // (two tiles at once spilled ~56 VGPRs of the walker state per env-step at 65,536 walkers)
  const pf4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
  for (int nt = 0; nt < NT; nt++) {
    float sB[3];
#pragma unroll
    for (int t = 0; t < 3; t++) sB[t] = tile[(16 * nt + n) * 16 + 4 * t + g];
    pf4 h1[4];
    float pv = 0.0f;
#pragma unroll
    for (int Mt = 0; Mt < 4; Mt++) {
      float wa[3], wc[3];
#pragma unroll
      for (int t = 0; t < 3; t++) {
        wa[t] = Wz[AW1F + (Mt * 3 + t) * 64 + lane];
        wc[t] = Wz[CW1F + (Mt * 3 + t) * 64 + lane];
      }
      const pf4 ba = *(const pf4*)(Wz + BA1 + 16 * Mt + 4 * g);
      const pf4 bc = *(const pf4*)(Wz + BC1 + 16 * Mt + 4 * g);
      const pf4 w2c = *(const pf4*)(Wz + WC2 + 16 * Mt + 4 * g);
      pf4 acc = z4, accc = z4;
#pragma unroll
      for (int t = 0; t < 3; t++) {
        acc = pmfma(wa[t], sB[t], acc);
        accc = pmfma(wc[t], sB[t], accc);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        h1[Mt][r] = plrelu(acc[r] + ba[r]);
        pv = pv + w2c[r] * plrelu(accc[r] + bc[r]);
      }
    }
    float p3[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int Mt = 0; Mt < 4; Mt++) {  // not unrolled: keeps one Mt's weights in flight
      pf4 acc = z4;
#pragma unroll
      for (int Mp = 0; Mp < 4; Mp++) {
        const pf4 w = *(const pf4*)(Wz + W2F + ((Mt * 4 + Mp) * 64 + lane) * 4);
#pragma unroll
        for (int r = 0; r < 4; r++) acc = pmfma(w[r], h1[Mp][r], acc);
      }
      const pf4 b2 = *(const pf4*)(Wz + BA2 + 16 * Mt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int k = 16 * Mt + 4 * g + r;
        const float h2 = plrelu(acc[r] + b2[r]);
#pragma unroll
        for (int d = 0; d < 4; d++) p3[d] = p3[d] + Wz[W3 + d * 64 + k] * h2;
      }
    }
    // the sums over the four lane groups (wk_mfma_layout.h: permlane swaps, the whole wave
    // active); lane (n, g) holds dim g's
    const float z3g = rows_rsum4(p3);
    pv = rows_sum4(pv);
    outs[(16 * nt + n) * 8 + g] = z3g;
    if (g == 0) outs[(16 * nt + n) * 8 + 4] = pv;
  }
  wave_lds_sync();  // the outputs are written before any lane reads its walker's
  const pf4 b3 = *(const pf4*)(Wz + BA3);
  const pf4 o = *(const pf4*)(outs + wl * 8);
#pragma unroll
  for (int d = 0; d < 4; d++) z3[d] = o[d] + b3[d];
  value = outs[wl * 8 + 4] + Wz[BC2];
  wave_lds_sync();  // outputs read before the next env-step rewrites the tile
}

constexpr int SIDE_BLOCK = SIDE_BLOCK_THREADS;  // 4 waves: the policy's weight image is staged once per block
// Q = 1: a lane pair per walker (L = 2); Q = 2: a lane quad (L = 4, side = lane bit 0, half =
// lane bit 1), for shards of at most one wave per SIMD, where the split shortens each wave's
// dependent chain -- with room for every register (one wave per SIMD: no spills)
template <bool POLICY, bool RECORD, bool TRACE, int Q, bool ROUGH = false>
__global__ __launch_bounds__(SIDE_BLOCK)
__attribute__((amdgpu_waves_per_eu(Q == 2 ? 1 : 2, Q == 2 ? 1 : 2)))  // (quad: one wave per SIMD)
void k_env_side(EnvParams P, StepArgs A) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int side = tid & 1;
  const int half = Q == 2 ? (tid >> 1) & 1 : 0;
  constexpr int SH = Q == 2 ? 2 : 1;  // log2 lanes per walker
  const int n = P.n_env;
  // sparse quad mapping (P.wpw < 16 walkers per wave, chosen so that one wave per SIMD still
  // holds every walker): the wave's first 4 wpw lanes hold wpw walkers, the other lanes replay
  // them (same walker, same branches, never store), so a wave's divergent branches are the
  // union over wpw walkers instead of sixteen
  const int wpw = Q == 2 ? P.wpw : 64 >> SH;  // (a power of two)
  const int eraw = ((tid >> 6) * wpw) + ((tid & ((wpw << SH) - 1)) >> SH);
  // a partial last wave keeps every lane (the policy's MFMAs need the whole wave):
  // out-of-range lanes replay walker n-1 and never store
  const bool active = eraw < n && (tid & 63) < (wpw << SH);
  // lane slot -> walker (wk_order.hip: episode-0 walkers first, so each wave's walkers visit
  // their floor pairs in one list order); every index below is the walker's own
  const int slot = eraw < n ? eraw : n - 1;
  const int e = A.order ? A.order[slot] : slot;
  const bool leader = side == 0 && half == 0 && active;
  __shared__ float pol_lds[POLICY ? (SIDE_BLOCK / 64) * 768 : 1];
  __shared__ float wz_lds[POLICY ? mf::WEND : 1];  // operand-order weights (41 KB, 2 blocks/CU)
  // RoughFloor: the walker's terrain heights 800 + Random.Next(0, 100) (Environment.cs:242-250),
  // [draw][walker of block]; the walker's lanes write the same values and read only its column
  constexpr int WPB = SIDE_BLOCK >> SH;
  __shared__ float ter_lds[ROUGH ? 11 * WPB : 1];
  // the pair mapping's contact faces (significant_face_lds): 6 records of 4 words per lane, as
  // one-word planes [word][lane of block] (24 KB per block; 2 blocks of 77 KB fit a CU's 160 KB -- not with the
  // rough floor's terrain as well, which would leave one block per CU).  The quad mapping keeps
  // the select chains (its LDS build: bit-exact, 1 % slower, profiles/r04_face_lds_ab.txt)
  constexpr int FS = (Q == 1 && !ROUGH) ? SIDE_BLOCK : 0;
  __shared__ float4 face_lds[FS ? 6 * SIDE_BLOCK : 1];
  // the rough floor's pair kernel has no face column (its terrain would push two blocks past the
  // CU's LDS); a 4-record column (16 KB per block, 2 x 75 KB fit) parks 16 of the legs' 24
  // vertex coordinates over the policy instead of leaving them to the spill
  constexpr int RS = (Q == 1 && ROUGH) ? SIDE_BLOCK : 0;
  __shared__ float4 rstash_lds[RS ? 4 * SIDE_BLOCK : 1];
  // the legs' stash across the policy section: the face column
  constexpr int SS = FS;
  const int wib = ((threadIdx.x >> 6) * wpw) + ((threadIdx.x & ((wpw << SH) - 1)) >> SH);
  const float* const ter = ter_lds + wib;
  if constexpr (ROUGH) {
#pragma unroll 1
    for (int i = 0; i < 11; i++)
      ter_lds[i * WPB + wib] = 800.0f + (float)terrain_draw(P.seed, (uint32_t)(P.env_offset + e), i);
  }
  if (POLICY) {
    for (int i = threadIdx.x; i < mf::WEND / 4; i += SIDE_BLOCK)
      ((pf4*)wz_lds)[i] = ((const pf4*)A.Wz)[i];
    __syncthreads();
  }
  SideState s;
  load_side(s, A.st, e, side);
  // (step_consts restated: through the helper these kernels compile to other code)
  const MatConst mc = material(A.mat[e]);
  const Mat mp{mc.inv_mass, 0.001f * mc.inv_mass, mc.restitution, mc.friction};
  const Mat mb{mc.inv_mass, 0.0003f, mc.restitution, mc.friction};  // Walker.cs:168
  const float dt = P.dt_sub;
  const float adx = 0.0f * dt, ady = 980.0f * dt;
  uint32_t t = A.rng_t[e];
  uint32_t fault = 0;
  RP_KERNEL_BEGIN(SIDE_BLOCK / 64);  // (probe builds only, wk_region_prof.h)

#pragma unroll 1
  for (int k = 0; k < A.k_steps; k++) {
    float a[4], lp[4], obs[12];
    if (Q == 1 && A.pace) pace_partner(A.pace, A.pace_seq, k);
    rp_mark(rp, RP_OTHER);
    // every LDS address of the env-step derived from the thread index afresh (an opaque copy
    // made inside the loop): hoisted out of the loop they were ten loop-invariant VGPRs that
    // the register allocator kept in scratch
    const int tx = (int)lane_opaque(threadIdx.x);
    // the lane's column of one-word planes: words (float*)face_lds + j * FS + tx, j < 24, for the
    // face records (significant_face_lds) and, over the policy, for the legs (park_legs_planes)
    float* const frec = (float*)face_lds + (FS ? tx : 0);
    float* const stash = frec;
    float* const wave_pol = pol_lds + (POLICY ? (tx >> 6) * 768 : 0);
    if (POLICY) {
      get_obs_side(s, side, obs);
      // The policy's matrix-core section needs the most registers of the loop, while the legs'
      // 24 vertex coordinates wait unused until the substeps: park them in this lane's contact-
      // face column (free outside the contact clipping) rather than leave them to the spill; the
      // empty asm with a memory clobber keeps the compiler from forwarding the parked values in
      // registers across the section.  Pure data movement: bit-identical.
      if constexpr (SS != 0) {
        park_legs_planes<SS>(s.lo, s.up, stash);
        asm volatile("" ::: "memory");
      } else if constexpr (RS != 0) {
        park_legs<RS, 4>(s, rstash_lds + tx);
        asm volatile("" ::: "memory");
      }
      float z3[4], mean[4], v;
      policy_mfma<Q>(wz_lds, obs, side == 0 && half == 0, wave_pol, z3, v, tx);
#pragma unroll
      for (int d = 0; d < 4; d++) mean[d] = tanhf(z3[d]);
      // (the walker's Philox counter word through an opaque copy: the first round's per-lane
      // products are recomputed per env-step rather than hoisted into seven spilled VGPRs)
      sample_actions(P, A.lp_const, (uint32_t)P.env_offset + lane_opaque((uint32_t)e), t, mean, a, lp);
      if (RECORD && leader) {  // the rows: 16-byte plain stores (st_row)
        // row base (uniform, SGPRs) + the lane's 32-bit offset (global_store saddr form): no
        // per-lane 64-bit pointer per array stays live across the env-step loop (they spilled)
        const size_t row = (size_t)(A.t0 + k) * n;
        const uint32_t eo = lane_opaque((uint32_t)e);
#pragma unroll
        for (int q = 0; q < 3; q++)
          st_row4(A.traj_s + row * 12 + (eo * 12u + 4u * q), obs[4 * q], obs[4 * q + 1], obs[4 * q + 2],
                  obs[4 * q + 3]);
        st_row4(A.traj_a + row * 4 + eo * 4u, a[0], a[1], a[2], a[3]);
        st_row4(A.traj_lp + row * 4 + eo * 4u, lp[0], lp[1], lp[2], lp[3]);
        st_row(v, A.traj_v + row + eo);
      }
      if constexpr (SS != 0) {
        asm volatile("" ::: "memory");
        unpark_legs_planes<SS>(s.lo, s.up, stash);
      } else if constexpr (RS != 0) {
        asm volatile("" ::: "memory");
        unpark_legs<RS, 4>(s, rstash_lds + tx);
      }
    } else {
#pragma unroll
      for (int d = 0; d < 4; d++) a[d] = A.actions[((size_t)k * n + e) * 4 + d];
    }
    rp_mark(rp, RP_POLICY);
    s.steps++;
    // Clip + Joint.SetTorque: joint `side` drives this upper leg, joint 2+side the lower
    {
      const float au = clip1(side ? a[1] : a[0]), al = clip1(side ? a[3] : a[2]);
      float c = au - s.tq_up; s.tq_up = au; s.dup.w = s.dup.w + c * 5.0f;
      c = al - s.tq_lo; s.tq_lo = al; s.dlo.w = s.dlo.w + c * 5.0f;
    }
#pragma unroll 1
    for (int it = 0; it < P.iterations; it++) {
      PairTraceDev* tr = (TRACE && active && half == 0) ? A.trace + ((size_t)e * P.iterations + it) : nullptr;
      substep_side<TRACE, Q, ROUGH, WPB, FS>(s, mp, mb, dt, adx, ady, tr, side, half, rp, ter, frec);
    }
    // Walker.Update + terminal flags (both upper legs and the torso)
    s.prevx = s.posx; s.prevy = s.posy;
    s.posx = s.body.cx; s.posy = s.body.cy;
    const bool other_cup = pswap(s.cup ? 1.0f : 0.0f) != 0.0f;
    if (s.cbody || s.cup || other_cup) s.terminal = true;
    float reward = 0.0f;  // (frame_outcome restated, for the same reason)
    float dX = s.posx - s.prevx;
    float yb = s.body.y[1];
    reward = reward + ((dX > 0.0f && ((yb / 500.0f) < 1.6f)) ? dX : 0.0f);
    reward = reward - (((yb / 500.0f) > 1.65f) ? -0.1f : 0.0f);
    bool terminal = false;
    if (s.terminal || s.steps > P.max_timesteps) {
      if (s.terminal) reward -= 40.0f;
      terminal = true;
    }
    if (s.posx > 900.0f) {
      reward += 80.0f;
      terminal = true;
    }
    if (!side_finite(s)) fault |= 1u;
    const size_t krow = (size_t)k * n;  // (uniform) + the lane's 32-bit offset, as above
    const uint32_t eo = lane_opaque((uint32_t)e);
    if (A.pos_out && leader) {
      A.pos_out[krow * 2 + eo * 2u] = s.posx;
      A.pos_out[krow * 2 + (eo * 2u + 1u)] = s.posy;
    }
    if (terminal) {
      int ep = s.episodes + 1;
      // (the start offset re-read here: a loop-invariant dx or the template's vertices from it
      // would otherwise stay live, i.e. in scratch, across the whole loop)
      make_template_side(s, A.dxoff[lane_opaque((uint32_t)e)]);
      s.post = true;
      s.episodes = ep;
    }
    if (A.obs_out) {
      get_obs_side(s, side, obs);
      if (leader) {
#pragma unroll
        for (int i = 0; i < 12; i++) A.obs_out[krow * 12 + (eo * 12u + i)] = obs[i];
      }
    }
    if (leader) {
      if (A.rew_out) A.rew_out[krow + eo] = reward;
      if (A.done_out) A.done_out[krow + eo] = terminal ? 1 : 0;
      if (RECORD) {
        const size_t row = (size_t)(A.t0 + k) * n;
        st_row(reward, A.traj_r + row + eo);
        st_row((uint8_t)(terminal ? 1 : 0), A.traj_d + row + eo);
      }
    }
    t++;
  }
  // (the side and its record offsets formed here again: kept from the loads they stayed in scratch)
  if (active && half == 0) store_side(s, A.st, lane_opaque((uint32_t)e), (int)(lane_opaque(threadIdx.x) & 1u));
  RP_KERNEL_END();
  fault |= (uint32_t)pswap((float)fault);
  if (leader) {
    const uint32_t eo = lane_opaque((uint32_t)e);  // (addresses formed here, not kept from the loads)
    A.rng_t[eo] = t;
    if (A.fault_out) A.fault_out[eo] |= fault;
  }
}

// host side: k_env_side is instantiated where this is
template <int Q, bool ROUGH>
static void launch_side(int mode, const EnvParams& P, const StepArgs& A, hipStream_t s) {
  const size_t lanes = Q == 2 ? ((size_t)P.n_env + P.wpw - 1) / P.wpw * 64 : (size_t)P.n_env * 2;
  dim3 blk(SIDE_BLOCK), grd((unsigned)((lanes + SIDE_BLOCK - 1) / SIDE_BLOCK));
  switch (mode) {
    case 0: hipLaunchKernelGGL((k_env_side<false, false, false, Q, ROUGH>), grd, blk, 0, s, P, A); break;
    case 1: hipLaunchKernelGGL((k_env_side<false, false, true, Q, ROUGH>), grd, blk, 0, s, P, A); break;
    case 2: hipLaunchKernelGGL((k_env_side<true, false, false, Q, ROUGH>), grd, blk, 0, s, P, A); break;
    default: hipLaunchKernelGGL((k_env_side<true, true, false, Q, ROUGH>), grd, blk, 0, s, P, A); break;
  }
}
}  // namespace wk
