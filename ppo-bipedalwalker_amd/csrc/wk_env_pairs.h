// wk_env_pairs.h -- what one substep of Environment.StepObjects is made of in every env-step
// kernel (device side): the joints (joint_step), a body's own step (integrate) and its candidate
// pairs against another walker part or the floor (resolve_pair, floor_pairs), with the quad
// mapping's split SAT / contact helpers.  The kernel families order them: substep
// (wk_env_lane.h), substep_side (wk_env_side.h), substep_scene (wk_env_scene.h).
#pragma once
#include "wk_env_state.h"
#include "wk_region_prof.h"

namespace wk {

// ---------------- quad mapping helpers (L = 4: two lanes per leg) ----------------
// The lane pair of a leg (halves 0 and 1: quad_perm [2,3,0,1] partners) holds the same leg
// state and splits the heavy halves of its pairs; each half ends with the other's results
// (DPP) combined in the reference's order, so both hold identical values throughout.
DEV float hswap(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
}
// per-lane selects as bit masks: a ?: between register copies can be folded by LLVM into a
// load through a selected address, which moves the polygons to scratch memory (cf. pick)
DEV float fsel(uint32_t m, float a, float b) { return __uint_as_float(bsel(m, a, __float_as_uint(b))); }
template <int N>
DEV Poly<N> psel(bool c, const Poly<N>& a, const Poly<N>& b) {
  const uint32_t m = c ? 0xffffffffu : 0u;
  Poly<N> r;
#pragma unroll
  for (int i = 0; i < N; i++) { r.x[i] = fsel(m, a.x[i], b.x[i]); r.y[i] = fsel(m, a.y[i], b.y[i]); }
  r.cx = fsel(m, a.cx, b.cx);
  r.cy = fsel(m, a.cy, b.cy);
  return r;
}
// AxisChecks(A's edges, B) on half 0 and AxisChecks(B's edges, A) on half 1, then
// SATCollision's order: A's axes first, B's best only when strictly smaller (axis_pass
// takes on temp < depth, so the sequential result is the first strict minimum over A's axes
// then B's).  P / AXP: this half's own polygon and its normalised axes (for its face).
template <int N>
DEV bool sat_split(const Poly<N>& A, const Poly<N>& B, int half, V2& normal, float& depth,
                   Poly<N>& P, EdgeAxes<N>& AXP) {
  P = psel(half != 0, B, A);
  const Poly<N> Q = psel(half != 0, A, B);
  bool sep = false;
  V2 nn = mk(0.0f, 0.0f);
  float dd = FLT_MAX;
  axis_pass<N, N, false, false, N, N == 6>(P, Q, sep, nn, dd, &AXP);  // (P: a walker pole)
  const float dd_o = hswap(dd), nx_o = hswap(nn.x), ny_o = hswap(nn.y);
  const float dA = half ? dd_o : dd, dB = half ? dd : dd_o;
  const V2 nA = half ? mk(nx_o, ny_o) : nn, nB = half ? nn : mk(nx_o, ny_o);
  const bool takeB = dB < dA;
  depth = net_minf(dA, dB);  // (a NaN on either half stays NaN: no collision, see axis_pass)
  normal = takeB ? nB : nA;
  const V2 dir = mk(B.cx - A.cx, B.cy - A.cy);
  if (vdot(dir, normal) > 0.0f) normal = vmul(normal, -1.0f);
  return depth > 0.0f;  // (no axis separates: see sat in wk_device.h)
}
// GetContactPoints with the two faces split: half 0 A's on the normal, half 1 B's on its
// negation (each from its own SAT axes), exchanged, then the clipping in both
template <int N, int FS = 0>  // FS > 0: the face through LDS (significant_face_lds, column frec)
DEV int contacts_split(const Poly<N>& P, const EdgeAxes<N>& AXP, int half, V2 normal, V2& c0,
                       V2& c1, float* frec = nullptr) {
  V2 fa, fb, fm, fd;
  if constexpr (FS > 0) significant_face_lds<N, FS>(P, AXP, half ? vneg(normal) : normal, frec, fa, fb, fm, fd);
  else significant_face_ax(P, AXP, half ? vneg(normal) : normal, fa, fb, fm, fd);
  const V2 oa = mk(hswap(fa.x), hswap(fa.y)), ob = mk(hswap(fb.x), hswap(fb.y));
  const V2 om = mk(hswap(fm.x), hswap(fm.y)), od = mk(hswap(fd.x), hswap(fd.y));
  const bool h = half != 0;
  return contact_clip(h ? oa : fa, h ? ob : fb, h ? om : fm, h ? od : fd,
                      h ? fa : oa, h ? fb : ob, h ? fm : om, h ? fd : od, normal, c0, c1);
}
// SAT of a leg segment against the flat floor with the segment's six axes split three and
// three (half 1 walks the segment from vertex 3: its edges 0..2 are edges 3..5, the same
// vertex set projected), then the floor's four closed-form axes in both; every axis of A
// ends up in AX on both halves (for A's contact face)
DEV bool sat_floor_split(const Poly<6>& A, const Poly<4>& F, float mnx, float mny, float mxx,
                         float mxy, int half, V2& normal, float& depth, EdgeAxes<6>& AX) {
  Poly<6> R;
  const uint32_t hm = half ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    R.x[i] = fsel(hm, A.x[(i + 3) % 6], A.x[i]);
    R.y[i] = fsel(hm, A.y[(i + 3) % 6], A.y[i]);
  }
  R.cx = A.cx;
  R.cy = A.cy;
  bool sep = false;
  V2 nn = mk(0.0f, 0.0f);
  float dd = FLT_MAX;
  EdgeAxes<6> own;
  axis_pass<6, 4, true, false, 3, true>(R, F, sep, nn, dd, &own);  // (R: the pole, maybe rotated by 3)
  const float dd_o = hswap(dd), nx_o = hswap(nn.x), ny_o = hswap(nn.y);
  const float d0 = half ? dd_o : dd, d1 = half ? dd : dd_o;
  const V2 n0 = half ? mk(nx_o, ny_o) : nn, n1 = half ? nn : mk(nx_o, ny_o);
  const bool take1 = d1 < d0;
  depth = net_minf(d0, d1);
  normal = take1 ? n1 : n0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float ox = hswap(own.x[i]), oy = hswap(own.y[i]);
    AX.x[i] = half ? ox : own.x[i];
    AX.y[i] = half ? oy : own.y[i];
    AX.x[i + 3] = half ? own.x[i] : ox;
    AX.y[i + 3] = half ? own.y[i] : oy;
  }
  floor_axis(-50.0f, 1050.0f, mnx, mxx, 1.0f, 0.0f, sep, normal, depth);
  floor_axis(900.0f, 1050.0f, mny, mxy, -0.0f, 1.0f, sep, normal, depth);
  floor_axis(-1050.0f, 50.0f, -mxx, -mnx, -1.0f, 0.0f, sep, normal, depth);
  floor_axis(-1050.0f, -900.0f, -mxy, -mny, -0.0f, -1.0f, sep, normal, depth);
  V2 dir = mk(F.cx - A.cx, F.cy - A.cy);
  if (vdot(dir, normal) > 0.0f) normal = vmul(normal, -1.0f);
  return depth > 0.0f;  // (see sat in wk_device.h)
}

// RigidBody.ResolveCollisions body for one (this=A, other=B) candidate
// (Bodies/RigidBody.cs:66-96); B may be the static floor.  GENERIC: B is a static floor
// polygon other than the flat box (a rough-floor segment): its bounding box, SAT and
// contact faces are evaluated in general, with Vector2.Normalize's NaN for a zero edge.
// H = 2: the quad mapping (sub = this lane's half): SAT axes and contact faces split over
// the leg's two lanes (leg-leg and leg-floor pairs of Poly<6> segments).
// FS > 0: the contact faces through this lane's LDS column frec (stride FS, the pair mapping)
template <int NA, int NB, bool BSTATIC, bool TRACE, int L, bool GENERIC = false, int H = 1, int FS = 0>
DEV void resolve_pair(Poly<NA>& A, Dyn& dA, const Mat& mA, Poly<NB>& B, Dyn& dB, const Mat& mB,
                      bool& colA, PairTraceDev* tr, int pi, int sub, RegionProf* rp = nullptr,
                      uint32_t* ec = nullptr, float* frec = nullptr) {
  static_assert(H == 1 || (L == 1 && !GENERIC && NA == 6 && NB == (BSTATIC ? 4 : 6)),
                "the quad split covers leg-leg and leg-floor pairs");
  static_assert(!BSTATIC || NB == 4, "the static body is the floor");
  static_assert(!GENERIC || BSTATIC, "generic static floor polygon");
  constexpr bool FLAT = BSTATIC && !GENERIC;
  constexpr int EVK = !BSTATIC ? 0 : (NA == 5 ? 2 : 1);  // leg-leg, leg-floor, torso-floor
  float mnx, mny, mxx, mxy;  // A's bounding box (the floor pass of sat_floor reuses it)
  aabb(A, mnx, mny, mxx, mxy);
  bool ov;
  if constexpr (FLAT) {
    ov = mnx < 1050.0f && mxx > -50.0f && mny < 1050.0f && mxy > 900.0f;  // floor box
  } else {
    float b0x, b0y, b1x, b1y;
    aabb(B, b0x, b0y, b1x, b1y);
    ov = mnx < b1x && mxx > b0x && mny < b1y && mxy > b0y;
  }
  rp_mark(rp, RP_AABB_LL + EVK, ov ? 1.0f : 0.0f);
  if (!ov) return;
  if (ec) ec[EV_AABB_LL + EVK]++;
  if (TRACE && tr && pi >= 0) tr->aabb_hit[pi] = 1;
  if (BSTATIC) colA = true;  // body._isFloor -> Collided = true (:75)
  V2 n;
  float depth;
  bool hit;
  // the one- and two-lane mappings keep both polygons' SAT axes for the contact faces
  constexpr bool KEEP = L == 1 && !GENERIC;
  EdgeAxes<NA> axa;
  EdgeAxes<NB> axb;
  Poly<NA> own;  // H = 2 leg-leg: this half's polygon (A or B) and its axes (in axa)
  if constexpr (H == 2 && FLAT) hit = sat_floor_split(A, B, mnx, mny, mxx, mxy, sub, n, depth, axa);
  else if constexpr (H == 2) hit = sat_split(A, B, sub, n, depth, own, axa);
  else if constexpr (L > 1) hit = sat_row<L>(A, B, sub, n, depth);
  // (a Poly<6> here is always a walker pole: A is a leg segment or the torso, B a leg segment
  // or a floor; scene props resolve in wk_env_scene.h)
  else if constexpr (FLAT) hit = sat_floor<NA, NA == 6>(A, B, mnx, mny, mxx, mxy, n, depth, &axa);
  else if constexpr (KEEP) hit = sat<NA, NB, false, true>(A, B, n, depth, &axa, &axb);
  else hit = sat<NA, NB, GENERIC, true>(A, B, n, depth);
  rp_mark(rp, RP_SAT_LL + EVK, depth, n.x, n.y, hit ? 1.0f : 0.0f);
  if (!hit) return;
  if (ec) ec[EV_SAT_LL + EVK]++;
  V2 c0, c1;
  int nc;
  if constexpr (H == 2 && !BSTATIC) nc = contacts_split<NA, FS>(own, axa, sub, n, c0, c1, frec);
  else if constexpr (KEEP && FLAT) nc = contact_points_floor<NA, FS>(A, axa, n, c0, c1, frec);
  else if constexpr (KEEP) nc = contact_points_ax<NA, NB, FS>(A, axa, B, axb, n, c0, c1, frec);
  else nc = contact_points<NA, NB, GENERIC>(A, B, n, c0, c1);
  rp_mark(rp, RP_CON_LL + EVK, c0.x, c0.y, c1.x, c1.y, (float)nc);
  if (TRACE && tr && pi >= 0) {
    tr->sat_hit[pi] = 1;
    tr->n_contacts[pi] = (uint8_t)nc;
    tr->normal[pi][0] = n.x;
    tr->normal[pi][1] = n.y;
    tr->depth[pi] = depth;
    if (nc > 0) { tr->contact[pi][0][0] = c0.x; tr->contact[pi][0][1] = c0.y; }
    if (nc > 1) { tr->contact[pi][1][0] = c1.x; tr->contact[pi][1][1] = c1.y; }
  }
  // MoveObjects (:99-113): A is never static here
  if (BSTATIC) {
    move(A, vmul(n, depth));
  } else {
    move(A, vdiv(vmul(n, depth), 2.0f));
    move(B, vdiv(vmul(vneg(n), depth), 2.0f));
  }
  // Impulses.ResolveCollisions (Impulses.cs:12-28)
  if (ec) ec[EV_CONTACTS] += (uint32_t)nc;
  if (nc == 0) return;
  if (ec) ec[EV_IMP_LL + EVK]++;
  float e = net_maxf(mA.e, mB.e);
  float mu = net_minf(mA.mu, mB.mu);
  V2 contact = nc == 2 ? vdiv(vadd(c0, c1), 2.0f) : c0;
  Body bA{A.cx, A.cy, &dA, mA.im, mA.ii};
  Body bB{B.cx, B.cy, &dB, mB.im, mB.ii};
  V2 rA, rB, rAF, rBF;
  V2 tangent = mk(-n.y, n.x);
  float j, jf;
  if constexpr (H == 2) {  // the normal impulse on half 0, the friction impulse on half 1
    const uint32_t hm = sub ? 0xffffffffu : 0u;
    const float mine = calc_impulse(bA, bB, contact, fsel(hm, mu, 1.0f + e),
                                    mk(fsel(hm, tangent.x, n.x), fsel(hm, tangent.y, n.y)), rA, rB);
    const float other = hswap(mine);
    j = fsel(hm, other, mine);
    jf = fsel(hm, mine, other);
    rAF = rA;  // (the lever arms do not depend on the direction)
    rBF = rB;
  } else {
    j = calc_impulse(bA, bB, contact, 1.0f + e, n, rA, rB);
    jf = calc_impulse(bA, bB, contact, mu, tangent, rAF, rBF);
  }
  if (TRACE && tr && pi >= 0) { tr->impulse[pi][0] = j; tr->impulse[pi][1] = jf; }
  apply_impulses<BSTATIC>(bA, bB, n, j, rA, rB);
  apply_impulses<BSTATIC>(bA, bB, tangent, jf, rAF, rBF);
  rp_mark(rp, RP_IMP_LL + EVK, dA.vx, dA.vy, dA.w, dB.vx, dB.vy, dB.w);
}

// Joint.Step (Objects/RigidBodies/Joint.cs:31-41); ResolveJoint swaps the bodies (:40)
template <int NA, int NB, int IA, int IB, bool TRACE>
DEV void joint_step(Poly<NA>& A, Dyn& dA, const Mat& mA, Poly<NB>& B, Dyn& dB, const Mat& mB,
                    PairTraceDev* tr, int ji, uint32_t* ec = nullptr) {
  V2 ab = vsub(mk(B.x[IB], B.y[IB]), mk(A.x[IA], A.y[IA]));
  float depth = vlen(ab);
  if (depth < 0.1f) return;
  if (ec) ec[EV_JOINT]++;
  // ab.Normalize(): ab * (1 / sqrt(x^2 + y^2)), and that sqrt is depth (same correctly
  // rounded sqrt of the same sum); rcp_core is 1.0f / d bit for bit on [2^-48, 2^64]
  const float rinv = depth <= 0x1p63f ? rcp_core(depth) : 1.0f / depth;
  ab = mk(ab.x * rinv, ab.y * rinv);
  move(A, vdiv(vmul(ab, depth), 2.0f));
  move(B, vdiv(vmul(vneg(ab), depth), 2.0f));
  V2 contact = vdiv(vadd(mk(A.x[IA], A.y[IA]), mk(B.x[IB], B.y[IB])), 2.0f);
  Body bJ{B.cx, B.cy, &dB, mB.im, mB.ii};  // manifold.BodyA = joint body B
  Body bI{A.cx, A.cy, &dA, mA.im, mA.ii};  // manifold.BodyB = joint body A
  V2 rA, rB;
  float j = calc_impulse(bJ, bI, contact, 1.0f + 1.0f, ab, rA, rB);
  if (TRACE && tr) { tr->joint_depth[ji] = depth; tr->joint_impulse[ji] = j; }
  apply_impulses<false>(bJ, bI, ab, j, rA, rB);
}

// RigidBody.StepLinearVelocity + StepAngularVelocity (RigidBody.cs:116-140)
template <int N>
DEV void integrate(Poly<N>& P, Dyn& D, float dt, float adx, float ady) {
  D.vx = D.vx + adx;
  D.vy = D.vy + ady;
  move(P, mk(D.vx * dt, D.vy * dt));
  D.th = D.th + D.w * dt;
  D.th = wrap_angle(D.th);
  rotate(P, D.w * dt);
}

// Environment.CreateRoughFloor (Environment.cs:230-261), segment k of 10 (movement 120):
// {(x, 1050), previousVector, (x, y), (x + 120, 1050)} with x = -50 + 120 k; the first
// previousVector is (-50, 800 + draw 0), so segment 0 has three vertices on x = -50 (and
// a zero edge when draws 0 and 1 are equal).  All coordinates are small integers (exact).
DEV void rough_segment(Poly<4>& f, int k, float yprev, float y) {
  const float x = -50.0f + 120.0f * (float)k;
  f.x[0] = x;                         f.y[0] = 1050.0f;
  f.x[1] = k == 0 ? x : x - 120.0f;   f.y[1] = yprev;
  f.x[2] = x;                         f.y[2] = y;
  f.x[3] = x + 120.0f;                f.y[3] = 1050.0f;
  find_centroid(f);
}

// a walker part's candidate pair(s) against the floor: the flat box (Environment.cs:211-226)
// or, with RoughFloor, the 10 static segments in list order (ter: this walker's 11 terrain
// heights in LDS, stride TS)
template <int N, bool TRACE, int L, bool ROUGH, int TS = 64>
DEV void floor_pairs(Poly<N>& P, Dyn& D, const Mat& m, bool& col, PairTraceDev* tr, int pi,
                     int sub, const float* ter, uint32_t* ec = nullptr) {
  Dyn dfl;
  zero_dyn(dfl);
  const Mat mf{0.0f, 0.0f, 0.3f, 1.0f};  // Metal, static: inverse mass/inertia 0
  if constexpr (ROUGH) {
    // Only the segments whose x-extent can reach the part's are visited: segment k spans
    // [x_k - 120, x_k + 120] (k = 0: from x_0), x_k = -50 + 120 k, so a segment with
    // x_k + 120 <= mnx or x_k - 120 >= mxx fails the pair's own bounding-box test; the range
    // below keeps one more segment on each side (rounding of the bound itself), so every
    // segment it leaves out is more than 100 px clear.  In list order as before; once the
    // part has moved (a resolved pair) the remaining segments are all visited, as the full
    // loop would test them against the moved part.  A non-finite or huge box: every segment.
    // With the lane order by start offset a part spans 3-5 segments of the 10.
    float mnx, mny, mxx, mxy;
    aabb(P, mnx, mny, mxx, mxy);
    int k = 0, kend = 9;
    if (mnx >= -1.0e6f && mxx <= 1.0e6f) {
      k = max(0, (int)floorf((mnx - 70.0f) * (1.0f / 120.0f)) - 1);
      kend = min(9, (int)floorf((mxx + 170.0f) * (1.0f / 120.0f)) + 1);
    }
#pragma unroll 1
    for (; k <= kend; k++) {
      Poly<4> seg;
      rough_segment(seg, k, ter[k * TS], ter[(k + 1) * TS]);
      const float cx0 = P.cx, cy0 = P.cy;
      resolve_pair<N, 4, true, TRACE, L, true>(P, D, m, seg, dfl, mf, col, tr, -1, sub, nullptr, ec);
      if (!(P.cx == cx0 && P.cy == cy0)) kend = 9;
    }
  } else {
    Poly<4> fl;
    floor_poly(fl);
    resolve_pair<N, 4, true, TRACE, L>(P, D, m, fl, dfl, mf, col, tr, pi, sub, nullptr, ec);
  }
}

}  // namespace wk
