// usim_contact.h -- the contact solve of the soft torso's top face: the rows of the contacts, their Delassus blocks, the warm start, the block Jacobi iteration
// with its line search, the wrench on the site and the impulses on the elements (DESIGN.md sections 4.1, 4.2).  contact_rows / contact_solve are what the 16-lane step
// kernels of usim_step16.h call; cone_local is also the visit of the full torso (usim_full.h).
// (included by usim_kernels.hip inside namespace usim, after the LDS layout, group_sync and group_bcast / half_bcast / quad_bcast, before usim_episode.h)
#pragma once

#define EB(off) lds[TB_WORDS + eb * GE_STRIDE + (off)]

// value of lane l ^ 8 of the DPP row (row_ror:8): "the other half of the row" of a 16-lane group
DI float row_ror8(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, true)); }
// value of lane l - D of the DPP row, zero in the first D lanes (row_shr:D)
template <int D> DI float row_shr(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x110 + D, 0xf, 0xf, true)); }
// Quad layout of a 16-lane group whose halves hold the same eight values (x of lane k and of lane 8 + k is X_k): quads 0 and 1 get X_0..3, quads 2 and 3 get X_4..7, so
// that quad_bcast serves both halves at once.  Lanes 4-11 take the value four lanes away (row_ror:4 under bank mask 0110; X has period eight, so the direction does not
// matter), lanes 0-3 and 12-15 keep their own: one move, and only copies -- the bits of X_k are those of the lane that formed it.
DI float quad_layout(float x) { const int ix = __float_as_int(x); return __int_as_float(__builtin_amdgcn_update_dpp(ix, ix, 0x124, 0xf, 0x6, false)); }

// sum over the lanes of a group, delivered to every lane (three or four DPP steps; lane k + 8 first, so that a 16-lane group whose halves carry the two contacts
// of a pair adds in the order of an 8-lane group that holds both in one lane: the same bits)
template <int G>
DI float group_allsum(float x) {
    if constexpr (G == 16) x += row_ror8(x);
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xf, 0xf, true));                         // row_half_mirror: k <-> 7 - k
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true));                          // quad_perm [1 0 3 2]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, true));                          // quad_perm [2 3 0 1]
    return x;
}

// Two floats per lane, handled by the packed float32 instructions of the part (v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32: both halves in one issue slot): with 8-lane
// groups a lane carries BOTH contacts of a probe-element pair, and their visits are the same instruction sequence on different data.  Every operation below is the
// scalar one per component (IEEE fma / mul / add; v_rcp, v_rsq, min, max and the selects run once per half), so a pair visited in one lane has the bits of a pair
// visited in lanes k and 8 + k of a 16-lane group.
typedef float v2f __attribute__((ext_vector_type(2)));
struct b2 { bool x, y; };
template <class T> struct LaneVec;
template <> struct LaneVec<float> {
    typedef bool mask;
    static DI float splat(float a) { return a; }
    static DI float fma(float a, float b, float c) { return fmaf(a, b, c); }
    static DI float rcp(float a) { return rcp_(a); }
    static DI float rsq(float a) { return rsq_(a); }
    static DI float max(float a, float b) { return fmaxf(a, b); }
    static DI float min(float a, float b) { return fminf(a, b); }
    static DI bool gt(float a, float b) { return a > b; }
    static DI bool lt(float a, float b) { return a < b; }
    static DI bool both(bool a, bool b) { return bool(int(a) & int(b)); }
    static DI float sel(bool c, float a, float b) { return c ? a : b; }
    static DI float hsum(float a) { return a; }                       // sum over the lane's virtual contacts, in their order
    static DI float nsum(float a) { return -a; }                      // minus that sum, as the scalar code accumulates it: (-a0) - a1
};
template <> struct LaneVec<v2f> {
    typedef b2 mask;
    static DI v2f splat(float a) { return (v2f)(a); }
    static DI v2f fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
    static DI v2f rcp(v2f a) { v2f r; r.x = rcp_(a.x); r.y = rcp_(a.y); return r; }
    static DI v2f rsq(v2f a) { v2f r; r.x = rsq_(a.x); r.y = rsq_(a.y); return r; }
    static DI v2f max(v2f a, v2f b) { v2f r; r.x = fmaxf(a.x, b.x); r.y = fmaxf(a.y, b.y); return r; }
    static DI v2f min(v2f a, v2f b) { v2f r; r.x = fminf(a.x, b.x); r.y = fminf(a.y, b.y); return r; }
    static DI b2 gt(v2f a, v2f b) { return b2{a.x > b.x, a.y > b.y}; }
    static DI b2 lt(v2f a, v2f b) { return b2{a.x < b.x, a.y < b.y}; }
    static DI b2 both(b2 a, b2 b) { return b2{bool(int(a.x) & int(b.x)), bool(int(a.y) & int(b.y))}; }
    static DI v2f sel(b2 c, v2f a, v2f b) { v2f r; r.x = c.x ? a.x : b.x; r.y = c.y ? a.y : b.y; return r; }
    static DI float hsum(v2f a) { return a.x + a.y; }
    static DI float nsum(v2f a) { return -a.x - a.y; }
};

// One contact's block of the Jacobi iteration (oracle: cone_local_solve): from the force f, the residual r of its three rows and its block B (regulariser included),
// a better force h of the cone |h_t| <= mu h_n for the block's own problem.
//   (1) ray: exact line minimisation along the current force, f <- (1 + x) f, x >= -1;
//   (2) second ray, always, from the new point and its residual: along (1, 0, 0) or, when friction alone makes a force pay (r_n < mu |r_t|), along
//       (1, -mu r_t / |r_t|), x2 >= 0 -- a contact whose force the first ray has taken to zero starts again within the same visit, and the visit is a continuous
//       function of its inputs (no switch that float32 and float64 could take differently);
//   (3) friction with the normal fixed: the minimiser of the tangential 2 x 2 problem on the disc |t| <= mu n, t = -(B_tt + lambda I)^-1 r~ in adjugate form, one
//       Newton step on the secular equation from the contact's lambda of the iteration before, radial clamp.
// T = float: one contact per lane; T = v2f: the two contacts of a pair (same block, own residual, force, cone and multiplier) in the two halves.
// Returns whether the contact has a friction disc (lambda is meaningful).
template <class T>
DI typename LaneVec<T>::mask cone_local(const T b00, const T b01, const T b02, const T b11, const T b12, const T b22, T r0, T r1, T r2,
                                        const T f0, const T f1, const T f2, const T mu, T& lam, T& h0, T& h1, T& h2) {
    typedef LaneVec<T> V;
    const T Bf0 = V::fma(b02, f2, V::fma(b01, f1, b00 * f0)), Bf1 = V::fma(b12, f2, V::fma(b11, f1, b01 * f0)), Bf2 = V::fma(b22, f2, V::fma(b12, f1, b02 * f0));
    const T vr = V::fma(f2, r2, V::fma(f1, r1, f0 * r0)), vBv = V::fma(f2, Bf2, V::fma(f1, Bf1, f0 * Bf0));
    // (a force below 1e-10 N is left to the second ray: the damped steps of the iteration shrink a force that has to vanish geometrically, and once f0^2 underflows in
    //  float32 the quotient is inf -- oracle: same threshold)
    const T x = V::sel(V::gt(f0, V::splat(1e-10f)), V::max(-vr * V::rcp(vBv), V::splat(-1.f)), V::splat(0.f));
    r0 = V::fma(x, Bf0, r0); r1 = V::fma(x, Bf1, r1); r2 = V::fma(x, Bf2, r2);
    T n0 = V::fma(x, f0, f0), n1 = V::fma(x, f1, f1), n2 = V::fma(x, f2, f2);
    const T rt2 = V::fma(r1, r1, r2 * r2);
    const T irt = V::rsq(V::max(rt2, V::splat(1e-30f))), rtn = rt2 * irt;
    const T sl = V::sel(V::both(V::gt(rt2, V::splat(0.f)), V::lt(r0, mu * rtn)), -mu * irt, V::splat(0.f));
    const T u1 = sl * r1, u2 = sl * r2;                                            // second direction (1, u1, u2)
    const T Bu0 = V::fma(b02, u2, V::fma(b01, u1, b00)), Bu1 = V::fma(b12, u2, V::fma(b11, u1, b01)), Bu2 = V::fma(b22, u2, V::fma(b12, u1, b02));
    const T ur = V::fma(u2, r2, V::fma(u1, r1, r0)), uBu = V::fma(u2, Bu2, V::fma(u1, Bu1, Bu0));
    const T x2 = V::max(-ur * V::rcp(uBu), V::splat(0.f));
    n0 += x2; n1 = V::fma(x2, u1, n1); n2 = V::fma(x2, u2, n2);
    r1 = V::fma(x2, Bu1, r1); r2 = V::fma(x2, Bu2, r2);
    // friction on the disc |t| <= mu n0
    const T lim = mu * n0;
    // (a friction disc below 1e-7 N is no friction: the multiplier of such a disc is ~ |r~| / lim, and beyond 1e10 the squares below leave float32 -- oracle: same threshold)
    const typename V::mask haslim = V::gt(lim, V::splat(1e-7f));
    const T q1 = r1 - V::fma(b12, n2, b11 * n1), q2 = r2 - V::fma(b22, n2, b12 * n1);
    T m11 = b11 + lam, m22 = b22 + lam, det = V::fma(m11, m22, -(b12 * b12));
    T a1 = V::fma(m22, q1, -(b12 * q2)), a2 = V::fma(m11, q2, -(b12 * q1));
    {
        const T aa = V::fma(a1, a1, a2 * a2);
        const T aAa = V::fma(m11 * a2, a2, V::fma(m22 * a1, a1, -2.f * b12 * a1 * a2));
        const T an = aa * V::rsq(V::max(aa, V::splat(1e-30f)));
        lam = V::max(V::fma(V::fma(-det, lim, an) * aa, V::rcp(V::max(lim * aAa, V::splat(1e-30f))), lam), V::splat(0.f));
    }
    m11 = b11 + lam; m22 = b22 + lam; det = V::fma(m11, m22, -(b12 * b12));
    a1 = V::fma(m22, q1, -(b12 * q2)); a2 = V::fma(m11, q2, -(b12 * q1));
    const T aa = V::fma(a1, a1, a2 * a2);
    const T sc = -V::min(lim * V::rsq(aa), V::rcp(det));                           // (v_min keeps the number when aa = 0 makes the product inf or NaN)
    h0 = n0; h1 = V::sel(haslim, a1 * sc, V::splat(0.f)); h2 = V::sel(haslim, a2 * sc, V::splat(0.f));
    return haslim;
}

// The same visit for ONE contact per lane (the 16-lane groups that CLONE), with the quantities of its two tangent rows carried as one two-float value from the start:
// bt = (b01, b02), bA = (b11, b12), bB = (b12, b22), bD = (b11, b22); rt, ft, ht = rows 1 and 2 of r, f, h.  Every component is the operation of cone_local<float> on
// the same operands in the same order (one IEEE fma, mul or add per half of a v_pk_*; the dot products, the rays and the multiplier stay scalar chains): the same bits.
// Stated on its own because the vectoriser packs cone_local<float> only after moving registers together and leaves half of these pairs scalar, and because
// cone_local<float> is also the full torso's visit, whose kernels keep their code.
DI bool cone_local_rows12(const float b00, const v2f bt, const v2f bA, const v2f bB, const v2f bD, float r0, v2f rt, const float f0, const v2f ft, const float mu,
                          float& lam, float& h0, v2f& ht) {
    typedef LaneVec<float> S;
    typedef LaneVec<v2f> P;
    const float b12 = bA.y;
    const float Bf0 = fmaf(bt.y, ft.y, fmaf(bt.x, ft.x, b00 * f0));
    const v2f Bft = P::fma(bB, P::splat(ft.y), P::fma(bA, P::splat(ft.x), bt * f0));
    const float vr = fmaf(ft.y, rt.y, fmaf(ft.x, rt.x, f0 * r0)), vBv = fmaf(ft.y, Bft.y, fmaf(ft.x, Bft.x, f0 * Bf0));
    const float x = S::sel(S::gt(f0, 1e-10f), S::max(-vr * S::rcp(vBv), -1.f), 0.f);
    r0 = fmaf(x, Bf0, r0); rt = P::fma(P::splat(x), Bft, rt);
    float n0 = fmaf(x, f0, f0);
    v2f nt = P::fma(P::splat(x), ft, ft);
    const float rt2 = fmaf(rt.x, rt.x, rt.y * rt.y);
    const float irt = S::rsq(S::max(rt2, 1e-30f)), rtn = rt2 * irt;
    const float sl = S::sel(S::both(S::gt(rt2, 0.f), S::lt(r0, mu * rtn)), -mu * irt, 0.f);
    const v2f u = sl * rt;                                                         // second direction (1, u)
    const float Bu0 = fmaf(bt.y, u.y, fmaf(bt.x, u.x, b00));
    const v2f But = P::fma(bB, P::splat(u.y), P::fma(bA, P::splat(u.x), bt));
    const float ur = fmaf(u.y, rt.y, fmaf(u.x, rt.x, r0)), uBu = fmaf(u.y, But.y, fmaf(u.x, But.x, Bu0));
    const float x2 = S::max(-ur * S::rcp(uBu), 0.f);
    n0 += x2; nt = P::fma(P::splat(x2), u, nt);
    rt = P::fma(P::splat(x2), But, rt);
    const float lim = mu * n0;
    const bool haslim = S::gt(lim, 1e-7f);
    const v2f qt = rt - P::fma(bB, P::splat(nt.y), bA * nt.x);
    v2f mt = bD + lam;                                                             // (m11, m22); the adjugate takes them swapped: an op_sel of the same register pair
    float det = fmaf(mt.x, mt.y, -(b12 * b12));
    v2f at = P::fma(mt.yx, qt, -(b12 * qt.yx));
    {
        const float aa = fmaf(at.x, at.x, at.y * at.y);
        const v2f ma = mt.yx * at;                                                 // (m22 a1, m11 a2)
        const float aAa = fmaf(ma.y, at.y, fmaf(ma.x, at.x, -2.f * b12 * at.x * at.y));
        const float an = aa * S::rsq(S::max(aa, 1e-30f));
        lam = S::max(fmaf(fmaf(-det, lim, an) * aa, S::rcp(S::max(lim * aAa, 1e-30f)), lam), 0.f);
    }
    mt = bD + lam; det = fmaf(mt.x, mt.y, -(b12 * b12));
    at = P::fma(mt.yx, qt, -(b12 * qt.yx));
    const float aa = fmaf(at.x, at.x, at.y * at.y);
    const float sc = -S::min(lim * S::rsq(aa), S::rcp(det));
    h0 = n0; ht = haslim ? at * sc : P::splat(0.f);
    return haslim;
}

// ---- set-up: the rows of a contact.  Contact k of an environment lives in the registers of lane k of its group: row directions w, Lambda^-1 w, element coupling g,
//      reference acceleration, regulariser; Km[c] = Linv[e_own][e_c] / m ----
// The arm-independent half for the lane that holds contact cl (own: the slot is filled; a lane without a contact gets zeros): everything the rows need from the record,
// the lattice tables and the element state.  It writes through references, so that contact_rows points it at the struct it hands over and contact_solve at its own locals.
// FLAT (contact_solve's SHORT): no divergent region and no zeros to join behind it.  A lane without a contact runs the owning lanes' straight-line code on a zero
// frame -- its record's normal, lever arm, element and depth and the two frame entries that are 1 at a zero normal are selected to zero (ten selects) --, so that w,
// vrel0 and kdist follow as zeros (of either sign) through the unchanged arithmetic, g is selected to +0 (it is published), and Rd, Km, ae0 are finite values of
// element 0 that nothing outside the lane reads (finite everywhere, exact zeros where they are summed).  An owning lane executes the
// operations of the other form on the same operands in the same order.
template <bool FLAT = false>
DI void contact_row_geometry(const float* lds, const int eb, const int cl, const bool own, const DevModel& M, const DevCfg& C, const int nc, const int* cel, const float vz,
                             float (&w)[3][6], float (&g)[3], float (&Rd)[3], float (&Km)[MAXC], float (&vrel0)[3], float& ae0, float& kdist) {
    if constexpr (!FLAT) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c) Km[c] = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            g[d] = 0.f; Rd[d] = 0.f; vrel0[d] = 0.f;
#pragma unroll
            for (int a = 0; a < 6; ++a) w[d][a] = 0.f;
        }
        ae0 = 0.f; kdist = 0.f;
    }
    if (FLAT || own) {
        const bool blank = FLAT && !own;                                  // FLAT, no contact in this lane: a zero frame
        const auto z = [&](const float x) { return blank ? 0.f : x; };    // (the value is read or formed by every lane, then selected: no branch around it)
        const int b = GE_CG + cl * CG_WORDS;                             // (cl < MAXC: a slot of the environment's record area, filled or stale)
        f3 nn = mk(z(EB(b + 0)), z(EB(b + 1)), z(EB(b + 2))), rr = mk(z(EB(b + 3)), z(EB(b + 4)), z(EB(b + 5)));
        const int eown = __float_as_int(EB(b + 6)), e = blank ? 0 : eown;
        const float dist = z(EB(b + 7));
        // tangent frame without a case distinction (Frisvad 2012: continuous except at n.z = -1; contact normals point from the element towards the probe,
        // and no element sits above it): the iterate of a fixed number of row-by-row sweeps depends on the frame, so float32 and float64 must not be able
        // to choose different ones (oracle: same lines)
        const float aa = -rcp_(1.f + nn.z), bb = nn.x * nn.y * aa;
        f3 t1 = mk(z(1.f + nn.x * nn.x * aa), bb, -nn.x);               // (z: the entry is 1 at a zero normal)
        f3 t2 = mk(bb, z(1.f + nn.y * nn.y * aa), -nn.y);
        f3 ax = mk(lds[TB_AXIS + 3 * e], lds[TB_AXIS + 3 * e + 1], lds[TB_AXIS + 3 * e + 2]);
        const float sde = EB(GE_SD + e);
        float xx = fminf(-dist * (1.0f / SI_WIDTH), 1.f);
        float yy = (xx < 0.5f) ? 2.f * xx * xx : 1.f - 2.f * (1.f - xx) * (1.f - xx);
        float dimp = SI_D0 + yy * (SI_DMAX - SI_D0);
        float kk = dimp * (1.0f / (SI_DMAX * SI_DMAX * SR_TC * SR_TC));
        float Rn = (1.f - dimp) * rcp_(dimp) * M.invw;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) { const float t = lds[TB_LINV + e * LROW + cel[c]] * (1.0f / ELEM_MASS); Km[c] = (c < nc) ? t : 0.f; }   // (cel[c] = 0 beyond the count: the read is always in range, and a select costs less than a branch around it)
        ae0 = EB(GE_A + e);
        kdist = kk * dist;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            f3 dir = (d == 0) ? nn : (d == 1 ? t1 : t2);
            f3 rx = cross(rr, dir);
            w[d][0] = dir.x; w[d][1] = dir.y; w[d][2] = dir.z; w[d][3] = rx.x; w[d][4] = rx.y; w[d][5] = rx.z;
            const float gd = -dot(dir, ax);
            g[d] = z(gd);                                                 // (published: +0 in a lane without a contact, whatever the signs of its zero frame)
            vrel0[d] = gd * sde - dir.z * vz;
            Rd[d] = (d == 0) ? Rn * C.rn_scale : Rn * (1.0f / IMPRATIO);    // (two colliding probe geoms: two equal normal rows in parallel = half the regulariser)
        }
    }
}
// The arm-dependent half: Lambda^-1 w (Li: Lambda^-1, packed lower 6 x 6) and the residual of every row at zero force, from the site acceleration / velocity of the
// unconstrained arm (alpha, vs).
// FLAT: every lane runs the chains; a lane without a contact gets Lambda^-1 w = +0 exactly (fma chains from +0 over finite Lambda^-1 and zero w) and a residual that
// stays in the lane.
template <bool FLAT = false>
DI void contact_row_residual(const bool own, const float* Li, const float* alpha, const float* vs, const float (&w)[3][6], const float (&g)[3], const float (&vrel0)[3],
                             const float ae0, const float kdist, float (&Liw)[3][6], float (&cres)[3]) {
    if constexpr (!FLAT) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            cres[d] = 0.f;
#pragma unroll
            for (int a = 0; a < 6; ++a) Liw[d][a] = 0.f;
        }
    }
    if (FLAT || own) {
        const float bcon = 2.0f / (SI_DMAX * SR_TC);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float vrel = vrel0[d], wa = 0.f;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                float s = 0.f;
#pragma unroll
                for (int bb = 0; bb < 6; ++bb) s = fmaf((a >= bb) ? Li[PK(a, bb)] : Li[PK(bb, a)], w[d][bb], s);
                Liw[d][a] = s;
                vrel = fmaf(w[d][a], vs[a], vrel);
                wa = fmaf(w[d][a], alpha[a], wa);
            }
            const float aref = -bcon * vrel - (d == 0 ? kdist : 0.f);
            cres[d] = fmaf(g[d], ae0, wa) - aref;             // residual of row d at zero force
        }
    }
}

// What contact_row_geometry forms, as the split kernel's lattice side hands it over: it runs contact_rows before hand-off (2), while the arm side still forms Lambda^-1.
struct ContactRows {
    float w[3][6], g[3], Rd[3], Km[MAXC], vrel0[3], ae0, kdist;
};
template <int G>
DI void contact_rows(float* lds, const int eb, const int gl, const DevModel& M, const DevCfg& C, const int nc, const int* cel, const float vz, ContactRows& P) {
    contact_row_geometry(lds, eb, gl, gl < nc, M, C, nc, cel, vz, P.w, P.g, P.Rd, P.Km, P.vrel0, P.ae0, P.kdist);
}

// ---- warm start ----
// Kept contact list of an environment (usim_config.warm_start; oracle: uso_env.warm_el / warm_fv / warm_lamv): the element of every contact slot of the previous
// physics step with the force and the friction multiplier of its two virtual contacts.  The lane that runs a slot's visits keeps its record -- T = float: 16-lane
// groups, contact A of slot k in lane k, contact B in lane 8 + k; T = v2f: 8-lane groups, both in lane k -- in registers from step to step of a multi-step launch and
// in the environment's warm rows in HBM (usim_device.h WARM_*: one layout for every mapping) across launches.  NoWarm: handles without a warm start carry nothing.
struct NoWarm {};
template <class T> struct WarmRec { int el; T f[3], lam; };
template <int G> struct WarmOf { typedef WarmRec<typename std::conditional<G == 16, float, v2f>::type> type; };
template <class T> DI void warm_clear(WarmRec<T>& r) { r.el = -1; r.f[0] = r.f[1] = r.f[2] = r.lam = LaneVec<T>::splat(0.f); }
DI void warm_clear(NoWarm&) {}
// an environment's warm rows <-> the records of its group's lanes (every lane of the group calls; 16-byte accesses)
DI void warm_load(const float* wp, const int gl, WarmRec<float>& r) {
    const float4 x = *reinterpret_cast<const float4*>(wp + WARM_F + 4 * gl);
    r.el = __float_as_int(wp[WARM_EL + (gl & 7)]); r.f[0] = x.x; r.f[1] = x.y; r.f[2] = x.z; r.lam = x.w;
}
DI void warm_load(const float* wp, const int gl, WarmRec<v2f>& r) {
    const float4 a = *reinterpret_cast<const float4*>(wp + WARM_F + 4 * gl), b = *reinterpret_cast<const float4*>(wp + WARM_F + 4 * (MAXC + gl));
    r.el = __float_as_int(wp[WARM_EL + gl]);
    r.f[0].x = a.x; r.f[1].x = a.y; r.f[2].x = a.z; r.lam.x = a.w; r.f[0].y = b.x; r.f[1].y = b.y; r.f[2].y = b.z; r.lam.y = b.w;
}
DI void warm_store(float* wp, const int gl, const WarmRec<float>& r) {
    *reinterpret_cast<float4*>(wp + WARM_F + 4 * gl) = make_float4(r.f[0], r.f[1], r.f[2], r.lam);
    if (gl < MAXC) wp[WARM_EL + gl] = __int_as_float(r.el);
}
DI void warm_store(float* wp, const int gl, const WarmRec<v2f>& r) {
    *reinterpret_cast<float4*>(wp + WARM_F + 4 * gl) = make_float4(r.f[0].x, r.f[1].x, r.f[2].x, r.lam.x);
    *reinterpret_cast<float4*>(wp + WARM_F + 4 * (MAXC + gl)) = make_float4(r.f[0].y, r.f[1].y, r.f[2].y, r.lam.y);
    wp[WARM_EL + gl] = __int_as_float(r.el);
}
// the rows of an environment whose episode begins: no kept contact (G lanes of a group; every word of the rows)
template <int G> DI void warm_rows_clear(float* wp, const int gl) {
    for (int v = gl; v < WARM_WORDS / 4; v += G) reinterpret_cast<float4*>(wp)[v] = (v < MAXC / 4) ? make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1)) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// The kept list goes through the environment's LDS block (words 0 .. 71, laid out as the warm rows; the Delassus records there have been read by every lane), a lane
// finds its contact's element among the eight kept ones and takes that slot's force and multiplier.  No match, no contact: zero, as in a cold start.  myel: the
// element of the lane's contact, which warm_keep files with the solved force.
template <class VT>
DI void warm_match(float* lds, const int eb, const int gl, const int cl, const bool own, const typename LaneVec<VT>::mask ownv, const WarmRec<VT>& wr, int& myel,
                   VT (&fv)[3], VT& lamv) {
    static_assert(WARM_WORDS <= GE_SD, "kept list overlays the rhs / staging area");
    myel = own ? __float_as_int(EB(GE_CG + cl * CG_WORDS + 6)) : -1;
    group_sync();
    warm_store(&EB(0), gl, wr);
    group_sync();
    const float4 k0 = *reinterpret_cast<const float4*>(&EB(WARM_EL)), k1 = *reinterpret_cast<const float4*>(&EB(WARM_EL + 4));
    const int kel[MAXC] = {__float_as_int(k0.x), __float_as_int(k0.y), __float_as_int(k0.z), __float_as_int(k0.w),
                           __float_as_int(k1.x), __float_as_int(k1.y), __float_as_int(k1.z), __float_as_int(k1.w)};
    int m = -1;
#pragma unroll
    for (int k = 0; k < MAXC; ++k) m = (own && kel[k] == myel) ? k : m;
    const bool hit = m >= 0;
    const int ms = hit ? m : 0;
    if constexpr (std::is_same<VT, float>::value) {
        const float4 x = *reinterpret_cast<const float4*>(&EB(WARM_F + 4 * ((gl & 8) + ms)));
        const bool take = hit && ownv;
        fv[0] = take ? x.x : 0.f; fv[1] = take ? x.y : 0.f; fv[2] = take ? x.z : 0.f; lamv = take ? x.w : 0.f;
    } else {
        const float4 xa = *reinterpret_cast<const float4*>(&EB(WARM_F + 4 * ms)), xb = *reinterpret_cast<const float4*>(&EB(WARM_F + 4 * (MAXC + ms)));
        const bool ta = hit && ownv.x, tb = hit && ownv.y;
        fv[0].x = ta ? xa.x : 0.f; fv[1].x = ta ? xa.y : 0.f; fv[2].x = ta ? xa.z : 0.f; lamv.x = ta ? xa.w : 0.f;
        fv[0].y = tb ? xb.x : 0.f; fv[1].y = tb ? xb.y : 0.f; fv[2].y = tb ? xb.z : 0.f; lamv.y = tb ? xb.w : 0.f;
    }
}
template <class VT, class MASK> DI void warm_match(float*, int, int, int, bool, MASK, const NoWarm&, int&, VT (&)[3], VT&) {}      // cold: the forces stay zero
// the lane's new record: its contact's element, the solved forces and multipliers (a virtual contact that does not exist holds zeros)
template <class VT> DI void warm_keep(WarmRec<VT>& wr, const int myel, const VT (&fv)[3], const VT lamv) { wr.el = myel; wr.f[0] = fv[0]; wr.f[1] = fv[1]; wr.f[2] = fv[2]; wr.lam = lamv; }
template <class VT> DI void warm_keep(NoWarm&, int, const VT (&)[3], VT) {}

// ---- Delassus blocks: B[k][d][d'] = d(residual of row d of this lane's contact) / d(force on row d' of contact k)
//      = w_d . Lambda^-1 w^k_d' + g_d Km[k] g^k_d' (+ the regulariser on the diagonal of the lane's own block); an iteration then needs three broadcasts per contact. ----
// Lane k publishes Lambda^-1 w^k (18 words) and g^k (3) once in the environment's LDS block (the right-hand-side / staging area is free by now); every lane then reads
// contact k's record with six 16-byte broadcast reads -- a quarter of the issue slots the 21 DPP broadcasts took.
DI void delassus_publish(float* lds, const int eb, const int gl, const float (&Liw)[3][6], const float (&g)[3]) {
    static_assert(MAXC * 24 <= GE_SD, "Delassus records overlay the rhs / staging area");
    if (gl < MAXC) {
        float4* pub = reinterpret_cast<float4*>(&EB(gl * 24));
        pub[0] = make_float4(Liw[0][0], Liw[0][1], Liw[0][2], Liw[0][3]); pub[1] = make_float4(Liw[0][4], Liw[0][5], Liw[1][0], Liw[1][1]);
        pub[2] = make_float4(Liw[1][2], Liw[1][3], Liw[1][4], Liw[1][5]); pub[3] = make_float4(Liw[2][0], Liw[2][1], Liw[2][2], Liw[2][3]);
        pub[4] = make_float4(Liw[2][4], Liw[2][5], g[0], g[1]); pub[5] = make_float4(g[2], 0.f, 0.f, 0.f);
    }
    group_sync();
}
DI void load_record(const float* lds, const int eb, const int k, float4 (&rk)[6]) {
    const float4* src = reinterpret_cast<const float4*>(&EB(k * 24));
#pragma unroll
    for (int v = 0; v < 6; ++v) rk[v] = src[v];
}
// the block of this lane's rows (w, g) against the contact whose record holds Lambda^-1 w^k (Lk) and g^k Km (gk)
DI void delassus_block(const float (&w)[3][6], const float (&g)[3], const float (&Lk)[3][6], const float (&gk)[3], float (&Bj)[3][3]) {
#pragma unroll
    for (int dd = 0; dd < 3; ++dd) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float r1 = fmaf(w[d][4], Lk[dd][4], fmaf(w[d][2], Lk[dd][2], w[d][0] * Lk[dd][0]));
            float r2 = fmaf(w[d][5], Lk[dd][5], fmaf(w[d][3], Lk[dd][3], w[d][1] * Lk[dd][1]));
            Bj[d][dd] = fmaf(g[d], gk[dd], r1 + r2);
        }
    }
}
// The same block with the two partial sums of an entry -- r1 over the even components, r2 over the odd ones -- as the two halves of one packed value: wp[d][p] =
// (w[d][2p], w[d][2p + 1]), Lk[dd][p] likewise, which is how a record's words arrive from its 16-byte reads (every row of Lambda^-1 w^k starts at an even word).  Each
// half is the chain of delassus_block on the same operands in the same order, then r1 + r2 and the coupling term: the same bits.  Stated on its own for the reason
// cone_local_rows12 is: left to the vectoriser the entries are packed across rows, after moving the operands together.
DI void delassus_block_pairs(const v2f (&wp)[3][3], const float (&g)[3], const v2f (&Lk)[3][3], const float (&gk)[3], float (&Bj)[3][3]) {
    typedef LaneVec<v2f> P;
#pragma unroll
    for (int dd = 0; dd < 3; ++dd) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const v2f r = P::fma(wp[d][2], Lk[dd][2], P::fma(wp[d][1], Lk[dd][1], wp[d][0] * Lk[dd][0]));
            Bj[d][dd] = fmaf(g[d], gk[dd], r.x + r.y);
        }
    }
}
// a lane's own diagonal block, regulariser included
struct Sym3 { float b00, b01, b02, b11, b12, b22; };
// B[k] WITHOUT the regulariser; written and read only under k < ncr (the iterations run exactly the wave's largest contact count: a slot beyond the count of some
// other environment holds stale words, unused).  The reads of the next record are in flight while a block is formed.
// CLONE: 16 lanes per environment, eight contact slots: lanes 8-15 would idle through the set-up.  They clone lanes 0-7 instead (lane 8 + k forms the same rows of
// contact k, at no cost: same instructions) and take half of the blocks off them: a lane keeps FOUR blocks (round 6).  Up to four contacts in the wave: both halves
// form blocks 0-3 (the same instructions: no cost).  More: lanes 0-7 form the blocks of contacts 0-3, lanes 8-15 those of contacts 4-7 -- and keep them (rounds 3-5
// rotated every block to the other half: 36 rotations, 72 selects and 36 more registers per lane; the iteration no longer needs them) -- each half then sums its own
// four products of an iteration and one rotation adds the halves (delassus_product).  A slot beyond an environment's count holds zeros (its lane published zero rows),
// so its block is exactly zero.  Everything that leaves contact_solve is masked to lanes 0-7 or to lane k: forces stay zero in the clones (only lane k keeps an
// increment), the wrench sum and the publications read lanes < MAXC.
// PAIRS: the blocks through delassus_block_pairs (contact_solve's SHORT).
template <bool CLONE, bool PAIRS, int NB>
DI void delassus_blocks(const float* lds, const int eb, const int gl, const int cl, const int ncr, const float (&w)[3][6], const float (&g)[3], const float (&Rd)[3],
                        const float (&Km)[MAXC], float (&B)[NB][3][3], Sym3& bd) {
    const bool upper = CLONE && gl >= 8 && ncr > 4;                      // this half forms the blocks of contacts 4-7 (ncr is wave-uniform)
    const int k0 = upper ? 4 : 0;
    bd = Sym3{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 rk[6];
    load_record(lds, eb, k0, rk);
    v2f wp[3][3];
    if constexpr (PAIRS) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { wp[d][0] = v2f{w[d][0], w[d][1]}; wp[d][1] = v2f{w[d][2], w[d][3]}; wp[d][2] = v2f{w[d][4], w[d][5]}; }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (j < ncr) {
            float Kmj = Km[j];
            if constexpr (CLONE) Kmj = upper ? Km[4 + j] : Km[j];
            const float gk[3] = {rk[4].z * Kmj, rk[4].w * Kmj, rk[5].x * Kmj};
            if constexpr (PAIRS) {
                const v2f Lk[3][3] = {{{rk[0].x, rk[0].y}, {rk[0].z, rk[0].w}, {rk[1].x, rk[1].y}}, {{rk[1].z, rk[1].w}, {rk[2].x, rk[2].y}, {rk[2].z, rk[2].w}},
                                      {{rk[3].x, rk[3].y}, {rk[3].z, rk[3].w}, {rk[4].x, rk[4].y}}};
                if (j + 1 < NB) load_record(lds, eb, k0 + j + 1, rk);
                delassus_block_pairs(wp, g, Lk, gk, B[j]);
            } else {
                const float Lk[3][6] = {{rk[0].x, rk[0].y, rk[0].z, rk[0].w, rk[1].x, rk[1].y}, {rk[1].z, rk[1].w, rk[2].x, rk[2].y, rk[2].z, rk[2].w},
                                        {rk[3].x, rk[3].y, rk[3].z, rk[3].w, rk[4].x, rk[4].y}};
                // (the record is unpacked here, before the next one's reads are issued into the same registers: delassus_block(w, g, rk, Kmj, B[j]) on a copy of the record
                //  or on one of two buffers put 1 - 12 more spilled registers into the single-wave 16-lane kernels: DESIGN.md section 10)
                if (j + 1 < NB) load_record(lds, eb, k0 + j + 1, rk);    // the next contact's record, in flight while this block is formed
                delassus_block(w, g, Lk, gk, B[j]);
            }
            // the lane's own diagonal block, if this half formed it (cl - k0 == j); otherwise the partner lane (the other half, same cl) did: one rotation below
            const bool me = (cl - k0) == j;
            bd.b00 = me ? B[j][0][0] : bd.b00; bd.b01 = me ? B[j][0][1] : bd.b01; bd.b02 = me ? B[j][0][2] : bd.b02;
            bd.b11 = me ? B[j][1][1] : bd.b11; bd.b12 = me ? B[j][1][2] : bd.b12; bd.b22 = me ? B[j][2][2] : bd.b22;
        }
    }
    if constexpr (CLONE) {
        if (ncr > 4) {                                                   // (exactly one lane of a pair holds the block, the other holds zeros: x + 0)
            bd.b00 += row_ror8(bd.b00); bd.b01 += row_ror8(bd.b01); bd.b02 += row_ror8(bd.b02);
            bd.b11 += row_ror8(bd.b11); bd.b12 += row_ror8(bd.b12); bd.b22 += row_ror8(bd.b22);
        }
    }
    bd.b00 += Rd[0]; bd.b11 += Rd[1]; bd.b22 += Rd[2];
}

// q = A D for the pairs' summed directions D (one per lane, D_k in lane k).  Up to four contacts: one running sum over them.  More: the sum over contacts 0-3 plus the
// sum over contacts 4-7 -- in that association in EVERY mapping (an environment's bits must not depend on its wave's neighbours: for one with at most four contacts
// the second sum is exact zeros) -- which a 16-lane group evaluates in its two halves at once: lanes 0-7 take D_j, lanes 8-15 D_(4+j) from the same row (two bank-masked
// broadcasts per word; QUAD: the row goes to the quad layout once per word, then one quad_perm per word and block serves both halves -- 15 moves instead of 24), each half
// multiplies with the four blocks it formed, one rotation by eight lanes adds the halves.  Eight contacts: 63 instructions (QUAD: 54) instead of 96 (round 5), six:
// 63 / 72.  Used by every iteration and, with a warm start, once before them (A s0): one statement of the association for both
// (a function template; as a lambda inside contact_solve the 8-lane split kernel of a cold handle spilled one more register).
template <int G, bool CLONE, bool QUAD, int NCM, int NB>
DI void delassus_product(const float (&B)[NB][3][3], const float D0, const float D1, const float D2, float& q0, float& q1, float& q2) {
    q0 = 0.f; q1 = 0.f; q2 = 0.f;
    if constexpr (NCM <= 4) {
#pragma unroll
        for (int k = 0; k < NCM; ++k) {
            const float e0 = group_bcast<G>(D0, k), e1 = group_bcast<G>(D1, k), e2 = group_bcast<G>(D2, k);
            q0 = fmaf(B[k][0][2], e2, fmaf(B[k][0][1], e1, fmaf(B[k][0][0], e0, q0)));
            q1 = fmaf(B[k][1][2], e2, fmaf(B[k][1][1], e1, fmaf(B[k][1][0], e0, q1)));
            q2 = fmaf(B[k][2][2], e2, fmaf(B[k][2][1], e1, fmaf(B[k][2][0], e0, q2)));
        }
    } else if constexpr (CLONE) {
        const float Q0 = QUAD ? quad_layout(D0) : D0, Q1 = QUAD ? quad_layout(D1) : D1, Q2 = QUAD ? quad_layout(D2) : D2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float e0 = QUAD ? quad_bcast(Q0, j) : half_bcast(D0, j), e1 = QUAD ? quad_bcast(Q1, j) : half_bcast(D1, j), e2 = QUAD ? quad_bcast(Q2, j) : half_bcast(D2, j);
            q0 = fmaf(B[j][0][2], e2, fmaf(B[j][0][1], e1, fmaf(B[j][0][0], e0, q0)));
            q1 = fmaf(B[j][1][2], e2, fmaf(B[j][1][1], e1, fmaf(B[j][1][0], e0, q1)));
            q2 = fmaf(B[j][2][2], e2, fmaf(B[j][2][1], e1, fmaf(B[j][2][0], e0, q2)));
        }
        q0 += row_ror8(q0); q1 += row_ror8(q1); q2 += row_ror8(q2);
    } else {
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
        for (int k = 0; k < NCM; ++k) {
            const float e0 = group_bcast<G>(D0, k), e1 = group_bcast<G>(D1, k), e2 = group_bcast<G>(D2, k);
            float& a0 = (k < 4) ? q0 : h0; float& a1 = (k < 4) ? q1 : h1; float& a2 = (k < 4) ? q2 : h2;
            a0 = fmaf(B[k][0][2], e2, fmaf(B[k][0][1], e1, fmaf(B[k][0][0], e0, a0)));
            a1 = fmaf(B[k][1][2], e2, fmaf(B[k][1][1], e1, fmaf(B[k][1][0], e0, a1)));
            a2 = fmaf(B[k][2][2], e2, fmaf(B[k][2][1], e1, fmaf(B[k][2][0], e0, a2)));
        }
        q0 += h0; q1 += h1; q2 += h2;
    }
}

// Virtual contacts per lane: one (VT = float, 16-lane groups that CLONE: contact A of pair k in lane k, contact B in lane 8 + k) or two (VT = v2f: both in lane k, in
// the two halves of packed registers -- one visit for the pair at the issue cost of ~1.2 instead of two: round 6).
template <bool CLONE> using ContactLane = typename std::conditional<CLONE, float, v2f>::type;

// ---- BLOCK JACOBI WITH AN EXACT LINE SEARCH on the dual  min 1/2 f'(A + R) f + b'f,  f_v in {|f_t| <= mu_v f_n}  (round 5; oracle: constrained_forward,
//      cone_solver 2 -- same optimum as the exact-cone Gauss-Seidel of round 4, i.e. MuJoCo's Newton solver's).  A Gauss-Seidel sweep is one visit per contact, one
//      after the other, in which one lane of sixteen does useful work -- and two visits per probe-element pair once its two coincident contacts
//      (ultrasound_probe_gripper.xml:8-9: probe_collision, mu 0.01 after MuJoCo's max rule, and probe_visual, mu 1) are modelled explicitly.  A wave issues one
//      instruction per ~4 cycles whatever its lanes do (profiles/r05/micro_two_wave.txt), so here EVERY virtual contact runs its visit at the same time: contact A of
//      pair k in lane k, contact B in lane 8 + k (16-lane groups; both in lane k with 8-lane groups), each on its own 3 x 3 block from the current residual
//      (cone_local: ray update with an immediate restart from zero, friction QCQP with one Newton step on the carried multiplier).  The step along d = f^ - f is
//      t = (sum_v d_v'B_v d_v) / (d'Qd) <= 1 (the exact minimiser of the quadratic when every block is solved exactly, never longer) -- a convex combination of feasible points, no projection --; the shared residual moves by t A D,
//      D_k = d_Ak + d_Bk (three row broadcasts and nine multiply-adds per pair: the only part that grows with the contact count).  `iters` iterations from the forces
//      fv and multipliers lamv (zero: cold start; WARM: the kept ones, and the shared residual cres first moves to them).  NCM: the wave's largest contact count ----
template <int G, bool CLONE, bool WARM, bool QUAD, bool PAIR, int NCM, int NB>
DI void jacobi_iterations(const int iters, const float (&B)[NB][3][3], const Sym3& bd, const float (&Rd)[3], const typename LaneVec<ContactLane<CLONE>>::mask ownv,
                          const ContactLane<CLONE> muv, ContactLane<CLONE> (&fv)[3], ContactLane<CLONE>& lamv, float (&cres)[3]) {
    typedef ContactLane<CLONE> VT;
    typedef LaneVec<VT> V;
    const VT vb00 = V::splat(bd.b00), vb01 = V::splat(bd.b01), vb02 = V::splat(bd.b02), vb11 = V::splat(bd.b11), vb12 = V::splat(bd.b12), vb22 = V::splat(bd.b22);
    const VT vR0 = V::splat(Rd[0]), vR1 = V::splat(Rd[1]), vR2 = V::splat(Rd[2]);
    if constexpr (WARM) {
        // the shared residual at the kept forces: b + A s0, s0 = f_A + f_B per pair -- one product
        float D0 = V::hsum(fv[0]), D1 = V::hsum(fv[1]), D2 = V::hsum(fv[2]);
        if constexpr (CLONE) { D0 += row_ror8(D0); D1 += row_ror8(D1); D2 += row_ror8(D2); }
        float q0, q1, q2;
        delassus_product<G, CLONE, QUAD, NCM>(B, D0, D1, D2, q0, q1, q2);
        cres[0] += q0; cres[1] += q1; cres[2] += q2;
    }
    if constexpr (PAIR) {
        static_assert(CLONE, "cone_local_rows12 visits one contact per lane");
        // one contact per lane: rows 1 and 2 as a pair (cone_local_rows12); the arithmetic of the general statement below, component by component
        typedef LaneVec<v2f> P;
        const v2f bt = {bd.b01, bd.b02}, bA = {bd.b11, bd.b12}, bB = {bd.b12, bd.b22}, bD = {bd.b11, bd.b22}, vRt = {Rd[1], Rd[2]};
        float f0 = fv[0], c0 = cres[0];
        v2f ft = {fv[1], fv[2]}, ct = {cres[1], cres[2]};
        for (int it = 0; it < iters; ++it) {
            float h0, lam = lamv;
            v2f ht;
            const bool haslim = cone_local_rows12(bd.b00, bt, bA, bB, bD, fmaf(Rd[0], f0, c0), P::fma(vRt, ft, ct), f0, ft, muv, lam, h0, ht);
            lamv = V::sel(V::both(ownv, haslim), lam, lamv);
            const float e0 = V::sel(ownv, h0 - f0, 0.f);
            const v2f et = ownv ? ht - ft : P::splat(0.f);
            const float Be0 = fmaf(bt.y, et.y, fmaf(bt.x, et.x, bd.b00 * e0));
            const v2f Bet = P::fma(bB, P::splat(et.y), P::fma(bA, P::splat(et.x), bt * e0));
            float num = -fmaf(et.y, Bet.y, fmaf(et.x, Bet.x, e0 * Be0));
            const float D0 = e0 + row_ror8(e0), D1 = et.x + row_ror8(et.x), D2 = et.y + row_ror8(et.y);
            float q0, q1, q2;
            delassus_product<G, CLONE, QUAD, NCM>(B, D0, D1, D2, q0, q1, q2);
            const v2f qt = {q1, q2}, wt = P::fma(vRt, et, qt);
            float den = fmaf(et.y, wt.y, fmaf(et.x, wt.x, e0 * fmaf(Rd[0], e0, q0)));
            num = group_allsum<G>(num); den = group_allsum<G>(den);
            const float t = (den > 0.f) ? fminf(-num * rcp_(den), 1.f) : 0.f;
            f0 = fmaf(t, e0, f0); ft = P::fma(P::splat(t), et, ft);
            c0 = fmaf(t, q0, c0); ct = P::fma(P::splat(t), qt, ct);
        }
        fv[0] = f0; fv[1] = ft.x; fv[2] = ft.y; cres[0] = c0; cres[1] = ct.x; cres[2] = ct.y;
    } else for (int it = 0; it < iters; ++it) {
        VT dv[3];
        float num, D0, D1, D2;
        {
            const VT r0 = V::fma(vR0, fv[0], V::splat(cres[0])), r1 = V::fma(vR1, fv[1], V::splat(cres[1])), r2 = V::fma(vR2, fv[2], V::splat(cres[2]));
            VT h0, h1, h2, lam = lamv;
            const typename V::mask haslim = cone_local<VT>(vb00, vb01, vb02, vb11, vb12, vb22, r0, r1, r2, fv[0], fv[1], fv[2], muv, lam, h0, h1, h2);
            lamv = V::sel(V::both(ownv, haslim), lam, lamv);
            dv[0] = V::sel(ownv, h0 - fv[0], V::splat(0.f)); dv[1] = V::sel(ownv, h1 - fv[1], V::splat(0.f)); dv[2] = V::sel(ownv, h2 - fv[2], V::splat(0.f));
            // slope of the cost along d, block by block: -d'B d (for the minimiser of a block r.d <= -d'B d, with equality inside the cone) -- a sum of squares
            // instead of r.d, whose products cancel to second order for a sliding contact and are float32 noise once |d| < 5e-3 N (oracle: same lines)
            const VT e0 = dv[0], e1 = dv[1], e2 = dv[2];
            const VT Be0 = V::fma(vb02, e2, V::fma(vb01, e1, vb00 * e0)), Be1 = V::fma(vb12, e2, V::fma(vb11, e1, vb01 * e0)), Be2 = V::fma(vb22, e2, V::fma(vb12, e1, vb02 * e0));
            num = V::nsum(V::fma(e2, Be2, V::fma(e1, Be1, e0 * Be0)));          // (no 0 + x: the compiler may not fold it -- signed zeros -- and an instruction here is paid 24 times per step)
            D0 = V::hsum(dv[0]); D1 = V::hsum(dv[1]); D2 = V::hsum(dv[2]);
        }
        if constexpr (CLONE) { D0 += row_ror8(D0); D1 += row_ror8(D1); D2 += row_ror8(D2); }       // D_k = d_Ak + d_Bk in both halves
        float q0, q1, q2;
        delassus_product<G, CLONE, QUAD, NCM>(B, D0, D1, D2, q0, q1, q2);
        float den = V::hsum(V::fma(dv[2], V::fma(vR2, dv[2], V::splat(q2)), V::fma(dv[1], V::fma(vR1, dv[1], V::splat(q1)), dv[0] * V::fma(vR0, dv[0], V::splat(q0)))));
        num = group_allsum<G>(num); den = group_allsum<G>(den);
        const float t = (den > 0.f) ? fminf(-num * rcp_(den), 1.f) : 0.f;
        fv[0] = V::fma(V::splat(t), dv[0], fv[0]); fv[1] = V::fma(V::splat(t), dv[1], fv[1]); fv[2] = V::fma(V::splat(t), dv[2], fv[2]);
        cres[0] = fmaf(t, q0, cres[0]); cres[1] = fmaf(t, q1, cres[1]); cres[2] = fmaf(t, q2, cres[2]);
    }
}

// ---- contact wrench on the site (accumulated in W) and impulse along each contact's element axis (gf[k]); lanes without a contact hold w = g = f = 0, i.e.
//      contribute zeros ----
template <int G, bool CLONE>
DI void contact_wrench(const int gl, const float (&w)[3][6], const float (&g)[3], const ContactLane<CLONE> (&fv)[3], float* W, float* gf) {
    // the pair's total force (lanes 0-7 of a 16-lane group that clones: contact A's own force plus contact B's from lane 8 + k)
    float f[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if constexpr (CLONE) f[d] = fv[d] + row_ror8(fv[d]);
        else f[d] = LaneVec<v2f>::hsum(fv[d]);
    }
    const float Fw[6] = {w[0][0] * f[0] + w[1][0] * f[1] + w[2][0] * f[2], w[0][1] * f[0] + w[1][1] * f[1] + w[2][1] * f[2],
                         w[0][2] * f[0] + w[1][2] * f[1] + w[2][2] * f[2], w[0][3] * f[0] + w[1][3] * f[1] + w[2][3] * f[2],
                         w[0][4] * f[0] + w[1][4] * f[1] + w[2][4] * f[2], w[0][5] * f[0] + w[1][5] * f[1] + w[2][5] * f[2]};
    const float gfo = (g[0] * f[0] + g[1] * f[1] + g[2] * f[2]) * (1.0f / ELEM_MASS);
    // the sum over the eight contact lanes is a shifted-add reduction over the DPP row (16 lanes per environment: lanes 8-15 are masked;
    // 8 lanes per environment: the shifts are fenced at the group boundary, same tree, same bits), the per-contact impulses are
    // group broadcasts
    auto shr_add = [&](float v, auto Dc) {
        constexpr int D = decltype(Dc)::value;
        float t = row_shr<D>(v);
        if constexpr (G == 8) t = (gl < D) ? 0.f : t;
        return v + t;
    };
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        float v = (gl < MAXC) ? Fw[a] : 0.f;
        v = shr_add(v, std::integral_constant<int, 1>{});
        v = shr_add(v, std::integral_constant<int, 2>{});
        v = shr_add(v, std::integral_constant<int, 4>{});
        W[a] += group_bcast<G>(v, 7);
    }
#pragma unroll
    for (int k = 0; k < MAXC; ++k) gf[k] = group_bcast<G>(gfo, k);          // (no test per slot: a lane without a contact holds zeros)
}

// Contact solve of one forward pass (called when some environment of the wave has a contact).  Inputs: contact records in LDS (collide_queue, contact_overflow),
// element indices cel[], the site-space operator Lambda^-1 (Li, packed lower 6 x 6), the site acceleration / velocity of the unconstrained arm (alpha, vs).  Outputs:
// net contact wrench on the site W[6] (accumulated) and the impulse gf[k] along each contact's element axis.
// PRE: the arm-independent half of the rows comes from contact_rows (P); otherwise it is formed here (vz and the records; P is not read), into locals: handing the
// rows through the struct cost the 16-lane split kernel 0.5 us per step.
// WR = WarmRec: the solve starts from the kept record `wr` of the lane (matched by element against this pass's contact list) and leaves the new one in it.
// SHORT: the shortened Jacobi pass of groups that CLONE -- three pieces, each switched by its own constant below (same bits with or without any of them; DESIGN.md
// section 10).  The split kernel asks for it; the single-wave 16-lane kernels, which run at the register limit and spill more with any of the three, do not.
// With it the Delassus blocks of the set-up are formed from packed pairs as well (BPAIR; same bits, the single-wave kernels keep their instruction streams), and the
// rows are formed without a divergent region (FLAT: a lane without a contact runs them on a zero frame; same bits again).
template <int G, bool PRE, bool SHORT, class WR>
DI void contact_solve(float* lds, const int eb, const int gl, const DevModel& M, const DevCfg& C, const int nc, const int ncmax, const int* cel,
                      const float* Li, const float* alpha, const float* vs, const float mu, const float vz, const ContactRows& P, float* W, float* gf,
                      unsigned long long* dbg, WR& wr) {
    constexpr bool WARM = !std::is_same<WR, NoWarm>::value;
    constexpr bool CLONE = (G == 16) && !PRE;                            // lanes 8-15 of a 16-lane group clone lanes 0-7: delassus_blocks
    constexpr int NB = CLONE ? 4 : MAXC;
    constexpr bool QUAD = CLONE && SHORT;                                // the summed directions in the quad layout: one DPP move per broadcast word (delassus_product)
    constexpr bool PAIR = CLONE && SHORT;                                // the tangent rows of a contact as one two-float value (cone_local_rows12)
    constexpr bool ONE = CLONE && SHORT;                                 // five to eight contacts: one instantiation of the iterations
    constexpr bool BPAIR = CLONE && SHORT;                               // the Delassus blocks from packed pairs of row components (delassus_block_pairs; set-up, not the pass)
    constexpr bool FLAT = CLONE && SHORT;                                // the rows without a divergent region (contact_row_geometry, contact_row_residual; set-up, not the pass)
    typedef ContactLane<CLONE> VT;
    typedef LaneVec<VT> V;
    const int cl = CLONE ? (gl & 7) : gl;
    const bool own = cl < nc;
    const bool pairB = C.pair != 0;
    const float muB = fmaxf(C.probe_fric2, C.elem_fric);
    typename V::mask ownv; VT muv;
    if constexpr (CLONE) { ownv = own && (gl < 8 || pairB); muv = (gl < 8) ? mu : muB; }
    else { ownv = b2{own, own && pairB}; muv.x = mu; muv.y = muB; }

    USIM_CSTAMP(dbg, 0);
    float w[3][6], g[3], Rd[3], Km[MAXC], vrel0[3], ae0, kdist, Liw[3][6], cres[3];
    if constexpr (PRE) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c) Km[c] = P.Km[c];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            g[d] = P.g[d]; Rd[d] = P.Rd[d]; vrel0[d] = P.vrel0[d];
#pragma unroll
            for (int a = 0; a < 6; ++a) w[d][a] = P.w[d][a];
        }
        ae0 = P.ae0; kdist = P.kdist;
    } else contact_row_geometry<FLAT>(lds, eb, cl, own, M, C, nc, cel, vz, w, g, Rd, Km, vrel0, ae0, kdist);
    contact_row_residual<FLAT>(own, Li, alpha, vs, w, g, vrel0, ae0, kdist, Liw, cres);
    USIM_STAMP(dbg, 9);
    USIM_CSTAMP(dbg, 1);
    float B[NB][3][3];
    Sym3 bd;
    delassus_publish(lds, eb, gl, Liw, g);
    delassus_blocks<CLONE, BPAIR>(lds, eb, gl, cl, ncmax, w, g, Rd, Km, B, bd);
    USIM_CSTAMP(dbg, 2);
    VT fv[3] = {V::splat(0.f), V::splat(0.f), V::splat(0.f)}, lamv = V::splat(0.f);
    int myel = -1;
    warm_match(lds, eb, gl, cl, own, ownv, wr, myel, fv, lamv);
    // (one straight-line instantiation per wave-uniform contact count; groups that CLONE run the same code for five to eight contacts -- four blocks per half,
    //  whatever the count -- and with ONE they share one)
    auto iterations = [&](auto NCM) { jacobi_iterations<G, CLONE, WARM, QUAD, PAIR, decltype(NCM)::value>(C.pgs_iters, B, bd, Rd, ownv, muv, fv, lamv, cres); };
    switch ((ONE && ncmax > 4) ? MAXC : ncmax) {
        case 1: iterations(std::integral_constant<int, 1>{}); break;
        case 2: iterations(std::integral_constant<int, 2>{}); break;
        case 3: iterations(std::integral_constant<int, 3>{}); break;
        case 4: iterations(std::integral_constant<int, 4>{}); break;
        case 5: if constexpr (!ONE) iterations(std::integral_constant<int, 5>{}); break;
        case 6: if constexpr (!ONE) iterations(std::integral_constant<int, 6>{}); break;
        case 7: if constexpr (!ONE) iterations(std::integral_constant<int, 7>{}); break;
        default: iterations(std::integral_constant<int, MAXC>{}); break;
    }
    warm_keep(wr, myel, fv, lamv);
    USIM_STAMP(dbg, 10);
    USIM_CSTAMP(dbg, 3);
    contact_wrench<G, CLONE>(gl, w, g, fv, W, gf);
    USIM_CSTAMP(dbg, 4);
}

#undef EB
