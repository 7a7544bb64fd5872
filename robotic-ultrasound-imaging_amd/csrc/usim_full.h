// usim_full.h -- the FULL torso (usim_config.torso = USIM_TORSO_FULL) as a HIP workload: the rest of SURVEY.md section 8 row a3.  All 270 shell elements of the
// 9 x 4 x 11 composite (soft_box.xml:9) are dynamic sliders on the free torso body that ultrasound.py:426-431 writes at reset; the body rests on the table through
// element-table contacts (ultrasound_arena.py:55-58, friction 1).  One convex problem with the arm, solved in its dual over the probe-element contacts (<= 8 pairs,
// two coincident contacts each) and the element-table contacts (~54 while the box rests) by a block Gauss-Seidel whose visit is the continuous local solve of the top-face
// model's iteration (cone_local), taken in full -- the oracle's full torso (oracle/usim_oracle.c constrained_forward_full / cone_pgs_dense) runs the same model in the same
// order of visits on dense matrices; this file is written independently of it.  The solve starts from the forces of the previous physics step (LATF_WTAB / LATF_WPROBE in the
// environment's lattice block): cold, 24 sweeps over ~54 coupled sticking contacts are nowhere near converged (profiles/r05/full_torso_convergence.txt).
//
// Mapping: ONE WAVE PER ENVIRONMENT (usim_step_kernel<2, 64, MODE>: the arm mathematics is replicated in the 64 lanes; the torso is what the
// lanes share).  Lane l owns elements 5 l .. 5 l + 4 (s, sdot in registers).
//   * Torso Hessian H = [M I, 0, m N; 0, I_b, 0; m N', 0, m L] (body frame: linear 3, angular 3, sliders 270; N = slide axes, L = (1 + w_fix) I + w_ten Laplacian of the
//     shell graph, degree <= 4).  K = H^-1 is never formed: with S = M I - m N L^-1 N' (3 x 3) and P = L^-1 N' (270 x 3, host, float64)
//         K (x_l, x_a, x_s) = (a_l, I_b^-1 x_a, y / m - P a_l),   y = L^-1 x_s,   a_l = S^-1 (x_l - N y),
//     and y comes from FULL_CG_ITERS steps of conjugate gradients on the sparse L (condition number 4.8: 20 steps leave 1e-8; five elements and their <= 4 neighbours
//     per lane, search direction shared through LDS) -- two solves per forward pass (smooth + equality accelerations; accelerations of the contact forces).
//   * Gauss-Seidel without the dense Delassus matrix (3 x 86 rows squared = 260 KB per environment): a contact's rows touch 6 body coordinates and one slider, so
//     the residual of a visit is rebuilt from running sums -- the body accelerations a_l, a_a of all contact forces so far (updated through S^-1, I_b^-1), the arm's
//     site acceleration Lambda^-1 sum w'f (probe contacts), and per contact j the slider acceleration v_j = (L^-1 g_s)[e_j] / m, pushed at every visit of a contact c
//     by L^-1[e_j][e_c] (one word per contact and lane from the 292 KB table in L2, loaded at the top of the visit, used at its end).
//   * A visit is scalar work (the 3 x 3 block's cone_local) replicated in the lanes: the step is a chain of (contacts x sweeps) visits, ~1 k cycles each; the table visits
//     are software-pipelined by hand (record and L^-1 words of the next contact are loaded during the current visit).
#pragma once
// (included by usim_kernels.hip inside namespace usim, after probe_sdf / group_sync / GroupGeom)

constexpr int NSH = 270;                      // shell elements (soft_box.xml:9 count="9 4 11")
constexpr int FE = 5;                         // elements per lane: element e = FE * lane + i  (64 * 5 = 320 >= 270; elements >= 270 do not exist: mass-less, zero everywhere)
constexpr int FNE = 64 * FE;
constexpr int FULL_CG_ITERS = 20;
// table block of a full-torso handle (DevModel::tables), words
constexpr int FT_POS = 0;                     // float [270][3] element surface point, body frame
constexpr int FT_AXIS = 816;                  // float [270][3] slide axis (radial)
constexpr int FT_NBR = 1632;                  // int   [320][4] shell neighbours (FNE - 1 = a word that is always zero: no neighbour)
constexpr int FT_P = 2912;                    // float [270][3] P = L^-1 N'
constexpr int FT_DIAG = 3728;                 // float [320]    diagonal of L (1 for elements that do not exist)
constexpr int FT_CONST = 4048;                // float [32]     S^-1 (9), I_b^-1 (9), M_tot, contact regulariser scale of an element-table contact
constexpr int FT_LINV = 4080;                 // float [270][272] L^-1
constexpr int FT_LROW = 272;
constexpr int FT_WORDS = FT_LINV + NSH * FT_LROW;
// state of the lattice region (environment-major, LATF_ENV_WORDS words per environment)
constexpr int LATF_S = 0, LATF_SD = 272, LATF_BODY = 544;     // s[270], sdot[270], body: position (3, base-centred world axes), quaternion w x y z, linear velocity (world), angular velocity (body frame)
// warm start of the contact solve (the forces of the previous physics step: element-table contacts by element, probe contacts by element and geom):
constexpr int LATF_WTAB = 560;                // float [270][4] force (normal, t1, t2) and friction multiplier of the element's table contact; zeros: none
constexpr int LATF_WPROBE = LATF_WTAB + 4 * NSH;   // int [8] elements of the probe contact slots (-1: empty), then float [16][4]: contacts A of slots 0-7, contacts B
constexpr int LATF_WARM_WORDS = 4 * NSH + 8 + 64;
constexpr int LATF_ENV_WORDS = LATF_WPROBE + 8 + 64;      // 1712
static_assert(LATF_ENV_WORDS % 4 == 0 && LATF_WTAB % 4 == 0 && (LATF_WPROBE + 8) % 4 == 0, "16-byte accesses");
constexpr int F_TOTAL_FULL = F_NSCALAR + LATF_ENV_WORDS;
// contacts
constexpr int FMAXT = 120;                    // element-table contacts kept (ascending element id; ~54 - 63 while the box rests; beyond: status bit 1)
constexpr int FREC = 44;                      // probe contact record (slots 0-7 contacts A, 8-15 their coincident contacts B; slot s is built by lane s): a[3][3] b[3][3] c[3] R[3] res0[3] B[6] mu e f[3] lam P[e]
enum FullRec : int { FR_A = 0, FR_B = 9, FR_C = 18, FR_R = 21, FR_RES = 24, FR_BD = 27, FR_MU = 33, FR_E = 34, FR_F = 35, FR_LAM = 38, FR_PE = 39 /* P[e] (3) */ };
constexpr int FTREC = 24;                     // table contact record (contact i is built by lane i % 64): the directions are the rows of R_b for all of them, b_d = rb x a_d
enum FullTRec : int { TR_RB = 0, TR_C = 3, TR_RES = 6, TR_BD = 9, TR_RN = 15, TR_E = 16 /* before the rows are built: e, distance, x, y of the collision */, TR_F = 17, TR_LAM = 20, TR_PE = 21 };
constexpr int FMAXCAND = 16;
// LDS of a workgroup (= one wave = one environment), words: 19.4 KB, eight environments per CU
constexpr int FL_P = 0;                       // [320] conjugate-gradient search direction / element accelerations
constexpr int FL_SD = 320;                    // [320] sdot
constexpr int FL_U = 640;                     // [320] k_t s + b_t sdot; later the slider forces of the contacts
constexpr int FL_REC = 960;                   // [16][FREC]
constexpr int FL_PW = FL_REC + 16 * FREC;     // [8][36] probe contacts: w[3][6], Lambda^-1 w [3][6]
constexpr int FL_CAND = FL_PW + 8 * 36;       // [FMAXCAND][8] n(3) p(3) e dist
constexpr int FL_TREC = FL_CAND + FMAXCAND * 8; // [FMAXT][FTREC]
constexpr int FL_WORDS = FL_TREC + FMAXT * FTREC;
static_assert(FL_WORDS * 4 * 8 <= 160 * 1024 && FMAXT <= 128, "eight environments per CU; two table contacts per lane");

template <> struct GroupGeom<64> {
    static constexpr int EPW = 1, WAVES = 1, EPB = 1, NT = 64, LDS_WORDS = FL_WORDS;
};

DI float wave_sum(float x) {
    // sum over the 64 lanes in a fixed order, delivered to every lane: four DPP steps inside the rows, then the four row sums
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true));      // quad_perm [1 0 3 2]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, true));      // quad_perm [2 3 0 1]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xf, 0xf, true));     // row_half_mirror
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xf, 0xf, true));     // row_mirror
    const int xi = __float_as_int(x);
    return (__int_as_float(__builtin_amdgcn_readlane(xi, 0)) + __int_as_float(__builtin_amdgcn_readlane(xi, 16))) +
           (__int_as_float(__builtin_amdgcn_readlane(xi, 32)) + __int_as_float(__builtin_amdgcn_readlane(xi, 48)));
}
DI float lane_value(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }   // l wave-uniform

// y = L^-1 b on the shell graph (every lane: its FE elements)
DI void full_cg(float* lds, const int lane, const int (&nb)[FE][4], const float (&dg)[FE], const float wten, const float (&b)[FE], float (&x)[FE]) {
    float r[FE], p[FE];
    float rr = 0.f;
#pragma unroll
    for (int i = 0; i < FE; ++i) { x[i] = 0.f; r[i] = b[i]; p[i] = b[i]; rr = fmaf(b[i], b[i], rr); }
    rr = wave_sum(rr);
    for (int it = 0; it < FULL_CG_ITERS; ++it) {
        group_sync();
#pragma unroll
        for (int i = 0; i < FE; ++i) lds[FL_P + FE * lane + i] = p[i];
        group_sync();
        float ap[FE], pap = 0.f;
#pragma unroll
        for (int i = 0; i < FE; ++i) {
            const float nsum = (lds[FL_P + nb[i][0]] + lds[FL_P + nb[i][1]]) + (lds[FL_P + nb[i][2]] + lds[FL_P + nb[i][3]]);
            ap[i] = fmaf(dg[i], p[i], -wten * nsum);
            pap = fmaf(p[i], ap[i], pap);
        }
        pap = wave_sum(pap);
        const float alpha = (pap > 0.f) ? rr * rcp_(pap) : 0.f;
        float rn = 0.f;
#pragma unroll
        for (int i = 0; i < FE; ++i) { x[i] = fmaf(alpha, p[i], x[i]); r[i] = fmaf(-alpha, ap[i], r[i]); rn = fmaf(r[i], r[i], rn); }
        rn = wave_sum(rn);
        const float beta = (rr > 0.f) ? rn * rcp_(rr) : 0.f;
        rr = rn;
#pragma unroll
        for (int i = 0; i < FE; ++i) p[i] = fmaf(beta, p[i], r[i]);
    }
}

DI void frisvad_(const f3 n, f3& t1, f3& t2) {
    const float aa = -rcp_(1.f + n.z), bb = n.x * n.y * aa;
    t1 = mk(1.f + n.x * n.x * aa, bb, -n.x); t2 = mk(bb, 1.f + n.y * n.y * aa, -n.y);
}
DI f3 mul3(const float* A, const f3 v) { return mk(fmaf(A[2], v.z, fmaf(A[1], v.y, A[0] * v.x)), fmaf(A[5], v.z, fmaf(A[4], v.y, A[3] * v.x)), fmaf(A[8], v.z, fmaf(A[7], v.y, A[6] * v.x))); }

struct FullBody { f3 p; float q[4]; f3 v, w; };       // free body: position (base-centred world axes), quaternion w x y z, linear velocity (world), angular velocity (body frame)

// One forward pass of the full torso.  In: element state (registers), body state, arm quantities (site pose, Lambda^-1 packed lower, site acceleration alpha and
// velocity vs of the unconstrained arm).  Out: site wrench W of the probe contacts, element accelerations acc[] (own elements), body acceleration ab (linear, angular;
// body frame), contact list.
DI void full_forward(float* lds, const int lane, const DevModel& M, const DevCfg& C, const float kst, const float kdmp, const float mu, const float (&s)[FE], const float (&sd)[FE],
                     const FullBody& Bd, const f3 Kx, const f3 Ksx, const f3 Ksy, const f3 Ksz, const float* Li, const float* alpha, const float* vs,
                     float* W, float (&acc)[FE], float* ab, int& ncon, int* con_el, int& overflow, const float* wst, float* wout) {
    // wst: this environment's lattice block (the warm start is read from it) or nullptr: cold start (reset passes); wout: where the next step's warm start goes, or nullptr
    const float* tb = M.tables;
    const int* tbi = reinterpret_cast<const int*>(M.tables);
    // body rotation (columns of R_b)
    const float qw = Bd.q[0], qx = Bd.q[1], qy = Bd.q[2], qz = Bd.q[3];
    const f3 r0 = mk(1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qw * qz), 2.f * (qx * qz + qw * qy));      // rows of R_b
    const f3 r1 = mk(2.f * (qx * qy + qw * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qw * qx));
    const f3 r2 = mk(2.f * (qx * qz - qw * qy), 2.f * (qy * qz + qw * qx), 1.f - 2.f * (qx * qx + qy * qy));
    auto to_world = [&](const f3 v) { return mk(dot(r0, v), dot(r1, v), dot(r2, v)); };
    auto to_body = [&](const f3 v) { return r0 * v.x + r1 * v.y + r2 * v.z; };
    float Sinv[9], Ibinv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Sinv[k] = tb[FT_CONST + k]; Ibinv[k] = tb[FT_CONST + 9 + k]; }
    const float mtot = tb[FT_CONST + 18], invw_table = tb[FT_CONST + 19];
    const float ztab = 0.8f - M.base[2];
    // ---- own elements: tables ----
    int nb[FE][4]; float dg[FE]; f3 ax[FE], pos[FE], Pe[FE];
    bool ex[FE];
#pragma unroll
    for (int i = 0; i < FE; ++i) {
        const int e = FE * lane + i;
        ex[i] = e < NSH;
        const int ec = ex[i] ? e : 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) nb[i][d] = tbi[FT_NBR + 4 * e + d];
        dg[i] = tb[FT_DIAG + e];
        ax[i] = mk(tb[FT_AXIS + 3 * ec], tb[FT_AXIS + 3 * ec + 1], tb[FT_AXIS + 3 * ec + 2]);
        pos[i] = mk(tb[FT_POS + 3 * ec], tb[FT_POS + 3 * ec + 1], tb[FT_POS + 3 * ec + 2]);
        Pe[i] = mk(tb[FT_P + 3 * ec], tb[FT_P + 3 * ec + 1], tb[FT_P + 3 * ec + 2]);
    }
    // ---- smooth + equality accelerations of the torso: a~ = K rhs ----
    const f3 gb = to_body(mk(0.f, 0.f, -GRAV));
    const float kfix = 1.0f / (SI_DMAX * SR_TC * SR_TC), bfix = 2.0f / (SI_DMAX * SR_TC);
    const float kten = kst * (1.0f / SI_DMAX), bten = kdmp * (1.0f / SI_DMAX);
    group_sync();
#pragma unroll
    for (int i = 0; i < FE; ++i) { lds[FL_U + FE * lane + i] = ex[i] ? fmaf(kten, s[i], bten * sd[i]) : 0.f; lds[FL_SD + FE * lane + i] = sd[i]; }
    group_sync();
    float rhs[FE], y[FE];
#pragma unroll
    for (int i = 0; i < FE; ++i) {
        const float ue = lds[FL_U + FE * lane + i];
        // tendon rows: sum over the element's neighbours of -(u_e - u_j); a missing neighbour reads the zero word, so its share is put back
        int nn = 0;
        float usum = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) { const bool has = nb[i][d] != FNE - 1; nn += has ? 1 : 0; usum += lds[FL_U + nb[i][d]]; }
        const float r = dot(ax[i], gb) - M.wfix * fmaf(bfix, sd[i], kfix * s[i]) - M.wten * fmaf((float)nn, ue, -usum);
        rhs[i] = ex[i] ? r : 0.f;
    }
    full_cg(lds, lane, nb, dg, M.wten, rhs, y);
    f3 at_l;
    {
        f3 ny = mk(0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < FE; ++i) ny = madd(ny, ax[i], ex[i] ? y[i] : 0.f);
        ny = mk(wave_sum(ny.x), wave_sum(ny.y), wave_sum(ny.z));
        at_l = mul3(Sinv, gb * mtot - ny * ELEM_MASS);
    }
    float at_s[FE];
#pragma unroll
    for (int i = 0; i < FE; ++i) at_s[i] = ex[i] ? y[i] - dot(Pe[i], at_l) : 0.f;
    group_sync();
#pragma unroll
    for (int i = 0; i < FE; ++i) lds[FL_P + FE * lane + i] = at_s[i];
    // ---- collision: every element against the table plane and the probe ----
    const f3 vb = to_body(Bd.v), wb = Bd.w;
    int ntc = 0, ncand = 0;
    overflow = 0;
    {
        bool hit_t[FE], hit_p[FE];
        float dist_t[FE], dist_p[FE], tt_p[FE];
        f3 cx_t[FE], nn_p[FE], cp_p[FE];
        const float bound = C.probe_r + C.probe_h + C.probe_hl + C.probe_hw + 2.f * ELEM_HL + 2.f * ELEM_R;
#pragma unroll
        for (int i = 0; i < FE; ++i) {
            const f3 loc = madd(pos[i], ax[i], s[i] - ELEM_R);
            const f3 tip = to_world(loc) + Bd.p, axw = to_world(ax[i]);
            // table: the lower of the capsule's two end spheres
            const bool inner = fmaf(-2.f * ELEM_HL, axw.z, tip.z) < tip.z;
            const f3 cx = madd(tip, axw, inner ? -2.f * ELEM_HL : 0.f);
            dist_t[i] = cx.z - ELEM_R - ztab; cx_t[i] = cx;
            hit_t[i] = ex[i] && dist_t[i] < 0.f;
            // probe
            hit_p[i] = false; dist_p[i] = 0.f; tt_p[i] = 0.f; nn_p[i] = mk(0.f, 0.f, 1.f); cp_p[i] = tip;
            const f3 rel = tip - Kx;
            if (ex[i] && !(dot(rel, rel) > bound * bound)) {
                const f3 p0 = mk(dot(Ksx, rel), dot(Ksy, rel), dot(Ksz, rel));
                const f3 uw = axw * (-2.f * ELEM_HL);
                const f3 us = mk(dot(Ksx, uw), dot(Ksy, uw), dot(Ksz, uw));
                f3 g0, g1, gs;
                (void)probe_sdf(C, p0, g0);
                (void)probe_sdf(C, p0 + us, g1);
                const float s0 = dot(g0, us), s1 = dot(g1, us);
                const float tt = clampf(-s0 * rcp_(fmaxf(s1 - s0, 0.f) + SHAFT_EPS), 0.f, 1.f);
                const float dist = probe_sdf(C, madd(p0, us, tt), gs) - ELEM_R;
                const f3 nrm = (Ksx * gs.x + Ksy * gs.y + Ksz * gs.z) * -1.f;
                hit_p[i] = dist < 0.f; dist_p[i] = dist; tt_p[i] = tt; nn_p[i] = nrm;
                cp_p[i] = madd(tip, uw, tt) + nrm * (ELEM_R + 0.5f * dist);
            }
        }
        // ascending element order = lane-major: slots from the ballots
        const unsigned long long lt = (1ull << lane) - 1ull;
        int pre_t = 0, pre_p = 0, tot_t = 0, tot_p = 0;
#pragma unroll
        for (int i = 0; i < FE; ++i) {
            const unsigned long long bt = __ballot(hit_t[i]), bp = __ballot(hit_p[i]);
            pre_t += __popcll(bt & lt); tot_t += __popcll(bt);
            pre_p += __popcll(bp & lt); tot_p += __popcll(bp);
        }
        group_sync();
#pragma unroll
        for (int i = 0; i < FE; ++i) {
            if (hit_t[i]) {
                if (pre_t < FMAXT) *reinterpret_cast<float4*>(&lds[FL_TREC + FTREC * pre_t + TR_E]) = make_float4(__int_as_float(FE * lane + i), dist_t[i], cx_t[i].x, cx_t[i].y);
                ++pre_t;
            }
            if (hit_p[i]) {
                if (pre_p < FMAXCAND) {
                    float4* rec = reinterpret_cast<float4*>(&lds[FL_CAND + 8 * pre_p]);
                    rec[0] = make_float4(nn_p[i].x, nn_p[i].y, nn_p[i].z, cp_p[i].x);
                    rec[1] = make_float4(cp_p[i].y, cp_p[i].z, __int_as_float(FE * lane + i), dist_p[i]);
                }
                ++pre_p;
            }
        }
        group_sync();
        if (tot_t > FMAXT) overflow |= 2;
        ntc = tot_t < FMAXT ? tot_t : FMAXT;
        if (tot_p > MAXC) overflow |= 1;
        ncand = tot_p < FMAXCAND ? tot_p : FMAXCAND;
    }
    // more penetrating elements than contact slots: keep the MAXC deepest (ties keep the lower id), ascending order kept.  (Every lane runs the same scalar edit.)
    int nc = ncand;
    if (ncand > MAXC) {
        unsigned alive = (1u << ncand) - 1u;
        for (int drop = ncand - MAXC; drop > 0; --drop) {
            int worst = -1; float wd = 0.f;
            for (int j = 0; j < ncand; ++j) {
                const float dj = lds[FL_CAND + 8 * j + 7];
                if (((alive >> j) & 1u) && (worst < 0 || dj >= wd)) { wd = dj; worst = j; }
            }
            alive &= ~(1u << worst);
        }
        // compact (lane j moves record j to its new slot)
        const bool mine = lane < ncand && ((alive >> lane) & 1u);
        const int slot = __popc(alive & ((1u << lane) - 1u));
        float4 a0 = make_float4(0, 0, 0, 0), a1 = a0;
        if (mine) { const float4* rec = reinterpret_cast<const float4*>(&lds[FL_CAND + 8 * lane]); a0 = rec[0]; a1 = rec[1]; }
        group_sync();
        if (mine) { float4* rec = reinterpret_cast<float4*>(&lds[FL_CAND + 8 * slot]); rec[0] = a0; rec[1] = a1; }
        group_sync();
        nc = MAXC;
    }
    ncon = nc;
#pragma unroll
    for (int k = 0; k < MAXC; ++k) con_el[k] = (k < nc) ? __float_as_int(lds[FL_CAND + 8 * k + 6]) : -1;
    const bool pairB = C.pair != 0;
    const int nv = nc + ntc;
#pragma unroll
    for (int a = 0; a < 6; ++a) W[a] = 0.f;
    f3 al = mk(0.f, 0.f, 0.f), aa = mk(0.f, 0.f, 0.f);            // body accelerations of the contact forces (body frame)
    // contacts this lane builds and whose slider acceleration v = (L^-1 g_s)[e] / m it carries: [0] probe slot `lane` (lanes 0-15), [1], [2] table contacts lane, lane + 64
    int ej[3] = {0, 0, 0};
    float vj[3] = {0.f, 0.f, 0.f};
    // rows of a table contact (normal +z, tangents x, y of the world; table static): the body-frame directions are the rows of R_b, the same for all of them
    const f3 ta[3] = {r2, r0, r1};
    if (nv > 0) {
        const float bcon = 2.0f / (SI_DMAX * SR_TC);
        const float mu_table = fmaxf(1.0f, C.elem_fric), muB = fmaxf(C.probe_fric2, C.elem_fric);
        auto impedance = [&](const float dist, float& kk, float& rn) {
            const float xx = fminf(-dist * (1.0f / SI_WIDTH), 1.f);
            const float yy = (xx < 0.5f) ? 2.f * xx * xx : 1.f - 2.f * (1.f - xx) * (1.f - xx);
            const float dimp = SI_D0 + yy * (SI_DMAX - SI_D0);
            kk = dimp * (1.0f / (SI_DMAX * SI_DMAX * SR_TC * SR_TC));
            rn = (1.f - dimp) * rcp_(dimp);
        };
        // ---- probe rows: slot = lane (0-7 contacts A, 8-15 their coincident contacts B) ----
        if (lane < 16 && (lane & 7) < nc && (lane < 8 || pairB)) {
            const int sl = lane, pc = lane & 7;
            const float4* cr = reinterpret_cast<const float4*>(&lds[FL_CAND + 8 * pc]);
            const float4 a0 = cr[0], a1 = cr[1];
            const f3 dir0 = mk(a0.x, a0.y, a0.z), cpos = mk(a0.w, a1.x, a1.y);
            const int e = __float_as_int(a1.z); const float dist = a1.w;
            ej[0] = e;
            f3 dir[3]; dir[0] = dir0; frisvad_(dir0, dir[1], dir[2]);
            float kk, rn; impedance(dist, kk, rn);
            const float Rn = rn * M.invw;
            const f3 rb = to_body(cpos - Bd.p), rs = cpos - Kx;
            const f3 axe = mk(tb[FT_AXIS + 3 * e], tb[FT_AXIS + 3 * e + 1], tb[FT_AXIS + 3 * e + 2]);
            const f3 pe = mk(tb[FT_P + 3 * e], tb[FT_P + 3 * e + 1], tb[FT_P + 3 * e + 2]);
            const f3 ke = mul3(Sinv, pe) * -1.f;                                                   // K[0:3][6 + e]
            const float kee = tb[FT_LINV + e * FT_LROW + e] * (1.0f / ELEM_MASS) - dot(pe, ke);    // K[6 + e][6 + e]
            const float sde = lds[FL_SD + e], ate = lds[FL_P + e];
            float* rec = &lds[FL_REC + sl * FREC];
            f3 av[3], bv[3]; float cv[3], wv[3][6], wl[3][6];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const f3 db = to_body(dir[d]);
                av[d] = db * -1.f; bv[d] = cross(rb, db) * -1.f; cv[d] = -dot(db, axe);            // relative motion = probe point - element point
                float vrel = dot(av[d], vb) + dot(bv[d], wb) + cv[d] * sde;
                float acc0 = dot(av[d], at_l) + cv[d] * ate;
                const f3 rx = cross(rs, dir[d]);
                wv[d][0] = dir[d].x; wv[d][1] = dir[d].y; wv[d][2] = dir[d].z; wv[d][3] = rx.x; wv[d][4] = rx.y; wv[d][5] = rx.z;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    float t = 0.f;
#pragma unroll
                    for (int b = 0; b < 6; ++b) t = fmaf((a >= b) ? Li[PK(a, b)] : Li[PK(b, a)], wv[d][b], t);
                    wl[d][a] = t;
                    vrel = fmaf(wv[d][a], vs[a], vrel); acc0 = fmaf(wv[d][a], alpha[a], acc0);
                }
                rec[FR_A + 3 * d] = av[d].x; rec[FR_A + 3 * d + 1] = av[d].y; rec[FR_A + 3 * d + 2] = av[d].z;
                rec[FR_B + 3 * d] = bv[d].x; rec[FR_B + 3 * d + 1] = bv[d].y; rec[FR_B + 3 * d + 2] = bv[d].z;
                rec[FR_C + d] = cv[d];
                rec[FR_R + d] = (d == 0) ? Rn * C.rn_scale : Rn * (1.0f / IMPRATIO);      // (merged pair model: two equal normal rows in parallel)
                rec[FR_RES + d] = acc0 + bcon * vrel + ((d == 0) ? kk * dist : 0.f);
            }
            int q = 0;                                                                     // diagonal block (regulariser included), packed 00 01 02 11 12 22
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int d2 = d; d2 < 3; ++d2) {
                    float t = dot(av[d], mul3(Sinv, av[d2])) + dot(bv[d], mul3(Ibinv, bv[d2])) + cv[d] * dot(ke, av[d2]) + cv[d2] * dot(ke, av[d]) + cv[d] * cv[d2] * kee;
#pragma unroll
                    for (int a = 0; a < 6; ++a) t = fmaf(wv[d][a], wl[d2][a], t);
                    if (d == d2) t += rec[FR_R + d];
                    rec[FR_BD + q] = t; ++q;
                }
            rec[FR_MU] = (sl < 8) ? mu : muB;
            rec[FR_E] = __int_as_float(e);
            float4 wf = make_float4(0.f, 0.f, 0.f, 0.f);                                    // warm start: the force this element's contact with this geom had a step ago
            if (wst) {
#pragma unroll
                for (int j = 0; j < MAXC; ++j) if (__float_as_int(wst[LATF_WPROBE + j]) == e) wf = *reinterpret_cast<const float4*>(&wst[LATF_WPROBE + 8 + 4 * ((sl >> 3) * 8 + j)]);
            }
            rec[FR_F] = wf.x; rec[FR_F + 1] = wf.y; rec[FR_F + 2] = wf.z; rec[FR_LAM] = wf.w;
            rec[FR_PE] = pe.x; rec[FR_PE + 1] = pe.y; rec[FR_PE + 2] = pe.z;
            if (sl < 8) {
                float* pw = &lds[FL_PW + 36 * sl];
#pragma unroll
                for (int d = 0; d < 3; ++d)
#pragma unroll
                    for (int a = 0; a < 6; ++a) { pw[6 * d + a] = wv[d][a]; pw[18 + 6 * d + a] = wl[d][a]; }
            }
        }
        // ---- table rows: contact i is built by lane i % 64 (its collision record sits in the words of its own row record) ----
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int ti = lane + 64 * k;
            if (ti < ntc) {
                float* rec = &lds[FL_TREC + ti * FTREC];
                const float4 a0 = *reinterpret_cast<const float4*>(&rec[TR_E]);
                const int e = __float_as_int(a0.x); const float dist = a0.y;
                const f3 cpos = mk(a0.z, a0.w, ztab + 0.5f * dist);
                ej[1 + k] = e;
                float kk, rn; impedance(dist, kk, rn);
                const float Rn = rn * invw_table;
                const f3 rb = to_body(cpos - Bd.p);
                const f3 axe = mk(tb[FT_AXIS + 3 * e], tb[FT_AXIS + 3 * e + 1], tb[FT_AXIS + 3 * e + 2]);
                const f3 pe = mk(tb[FT_P + 3 * e], tb[FT_P + 3 * e + 1], tb[FT_P + 3 * e + 2]);
                const f3 ke = mul3(Sinv, pe) * -1.f;
                const float kee = tb[FT_LINV + e * FT_LROW + e] * (1.0f / ELEM_MASS) - dot(pe, ke);
                const float sde = lds[FL_SD + e], ate = lds[FL_P + e];
                f3 bv[3]; float cv[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    bv[d] = cross(rb, ta[d]); cv[d] = dot(ta[d], axe);
                    const float vrel = dot(ta[d], vb) + dot(bv[d], wb) + cv[d] * sde;
                    const float acc0 = dot(ta[d], at_l) + cv[d] * ate;
                    rec[TR_C + d] = cv[d];
                    rec[TR_RES + d] = acc0 + bcon * vrel + ((d == 0) ? kk * dist : 0.f);
                }
                int q = 0;
#pragma unroll
                for (int d = 0; d < 3; ++d)
#pragma unroll
                    for (int d2 = d; d2 < 3; ++d2) {
                        float t = dot(ta[d], mul3(Sinv, ta[d2])) + dot(bv[d], mul3(Ibinv, bv[d2])) + cv[d] * dot(ke, ta[d2]) + cv[d2] * dot(ke, ta[d]) + cv[d] * cv[d2] * kee;
                        if (d == d2) t += (d == 0) ? Rn : Rn * (1.0f / IMPRATIO);
                        rec[TR_BD + q] = t; ++q;
                    }
                rec[TR_RB] = rb.x; rec[TR_RB + 1] = rb.y; rec[TR_RB + 2] = rb.z;
                rec[TR_RN] = Rn;
                const float4 wf = wst ? *reinterpret_cast<const float4*>(&wst[LATF_WTAB + 4 * e]) : make_float4(0.f, 0.f, 0.f, 0.f);       // warm start (zeros: no table contact a step ago)
                rec[TR_E] = __int_as_float(e); rec[TR_F] = wf.x; rec[TR_F + 1] = wf.y; rec[TR_F + 2] = wf.z;
                rec[TR_LAM] = wf.w; rec[TR_PE] = pe.x; rec[TR_PE + 1] = pe.y; rec[TR_PE + 2] = pe.z;
            }
        }
        group_sync();
        // ---- block Gauss-Seidel, order: probe contacts A, table contacts, probe contacts B; pgs_iters sweeps, cold start ----
        auto visit = [&](const float b00, const float b01, const float b02, const float b11, const float b12, const float b22, float (&r)[3], const float (&f)[3],
                         const float muv, float& lam, float (&fc)[3]) {
            // cone_local (usim_kernels.hip), the continuous local solve of the top-face model's iteration, taken in full (Gauss-Seidel: no line search)
            float lam_new = lam;
            const bool haslim = cone_local(b00, b01, b02, b11, b12, b22, r[0], r[1], r[2], f[0], f[1], f[2], muv, lam_new, fc[0], fc[1], fc[2]);
            lam = haslim ? lam_new : lam;
        };
        // push of a visit: the body accelerations through S^-1 / I_b^-1, the slider acceleration of every contact through its word of row e of L^-1
        auto push = [&](const f3 dgl, const f3 dga, const float sig, const f3 pe, const float lj0, const float lj1, const float lj2) {
            al = al + mul3(Sinv, dgl - pe * sig);
            aa = aa + mul3(Ibinv, dga);
            const float sm = sig * (1.0f / ELEM_MASS);
            vj[0] = fmaf(lj0, sm, vj[0]); vj[1] = fmaf(lj1, sm, vj[1]); vj[2] = fmaf(lj2, sm, vj[2]);
        };
        float zw[6] = {0, 0, 0, 0, 0, 0};                            // site acceleration of the probe contact forces: Lambda^-1 sum w'f
        // init: the pass before the first sweep -- the running sums take up the warm-start forces (df = f, nothing is solved, nothing rewritten)
        auto probe_visit = [&](const int sl, const bool init) {
            float* rec = &lds[FL_REC + sl * FREC];
            float rw[FREC], pwv[36];
            {
                const float4* r4 = reinterpret_cast<const float4*>(rec);
#pragma unroll
                for (int k = 0; k < FREC / 4; ++k) { const float4 t = r4[k]; rw[4 * k] = t.x; rw[4 * k + 1] = t.y; rw[4 * k + 2] = t.z; rw[4 * k + 3] = t.w; }
                const float4* p4 = reinterpret_cast<const float4*>(&lds[FL_PW + 36 * (sl & 7)]);
#pragma unroll
                for (int k = 0; k < 9; ++k) { const float4 t = p4[k]; pwv[4 * k] = t.x; pwv[4 * k + 1] = t.y; pwv[4 * k + 2] = t.z; pwv[4 * k + 3] = t.w; }
            }
            const int e = __float_as_int(rw[FR_E]);
            const float lj0 = tb[FT_LINV + e * FT_LROW + ej[0]], lj1 = tb[FT_LINV + e * FT_LROW + ej[1]], lj2 = tb[FT_LINV + e * FT_LROW + ej[2]];    // (asked for now, used at the end)
            const f3 pe = mk(rw[FR_PE], rw[FR_PE + 1], rw[FR_PE + 2]);
            const float as_e = lane_value(vj[0], sl) - dot(pe, al);
            const float f[3] = {rw[FR_F], rw[FR_F + 1], rw[FR_F + 2]};
            f3 av[3], bv[3]; float cv[3], r[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                av[d] = mk(rw[FR_A + 3 * d], rw[FR_A + 3 * d + 1], rw[FR_A + 3 * d + 2]);
                bv[d] = mk(rw[FR_B + 3 * d], rw[FR_B + 3 * d + 1], rw[FR_B + 3 * d + 2]);
                cv[d] = rw[FR_C + d];
                float t = fmaf(rw[FR_R + d], f[d], rw[FR_RES + d]) + dot(av[d], al) + dot(bv[d], aa) + cv[d] * as_e;
#pragma unroll
                for (int a = 0; a < 6; ++a) t = fmaf(pwv[6 * d + a], zw[a], t);
                r[d] = t;
            }
            float fc[3] = {f[0], f[1], f[2]}, lam = rw[FR_LAM];
            float df[3] = {f[0], f[1], f[2]};
            if (!init) {
                visit(rw[FR_BD], rw[FR_BD + 1], rw[FR_BD + 2], rw[FR_BD + 3], rw[FR_BD + 4], rw[FR_BD + 5], r, f, rw[FR_MU], lam, fc);
                df[0] = fc[0] - f[0]; df[1] = fc[1] - f[1]; df[2] = fc[2] - f[2];
                *reinterpret_cast<float4*>(&rec[FR_F - 3]) = make_float4(rw[FR_F - 3], rw[FR_F - 2], rw[FR_F - 1], fc[0]);      // (words 32-35: B[5], mu, e, f0)
                *reinterpret_cast<float4*>(&rec[FR_F + 1]) = make_float4(fc[1], fc[2], lam, rw[FR_PE]);                            // (words 36-39: f1, f2, lambda, P[e].x)
            }
            push(av[0] * df[0] + av[1] * df[1] + av[2] * df[2], bv[0] * df[0] + bv[1] * df[1] + bv[2] * df[2], cv[0] * df[0] + cv[1] * df[1] + cv[2] * df[2], pe, lj0, lj1, lj2);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                zw[a] += pwv[18 + a] * df[0] + pwv[24 + a] * df[1] + pwv[30 + a] * df[2];
                W[a] += pwv[a] * df[0] + pwv[6 + a] * df[1] + pwv[12 + a] * df[2];
            }
            group_sync();
        };
        auto load_trec = [&](const int ti, float (&rw)[FTREC], float (&lj)[3]) {
            const float4* r4 = reinterpret_cast<const float4*>(&lds[FL_TREC + ti * FTREC]);
#pragma unroll
            for (int k = 0; k < FTREC / 4; ++k) { const float4 t = r4[k]; rw[4 * k] = t.x; rw[4 * k + 1] = t.y; rw[4 * k + 2] = t.z; rw[4 * k + 3] = t.w; }
            // (the element from the lane that built the contact, not from the record: the global addresses do not wait for LDS)
            const int e = __builtin_amdgcn_readlane((ti < 64) ? ej[1] : ej[2], ti & 63);
#pragma unroll
            for (int k = 0; k < 3; ++k) lj[k] = tb[FT_LINV + e * FT_LROW + ej[k]];
        };
        auto table_visit = [&](const int ti, const float (&rw)[FTREC], const float (&lj)[3], const bool init) {
            float* rec = &lds[FL_TREC + ti * FTREC];
            const f3 pe = mk(rw[TR_PE], rw[TR_PE + 1], rw[TR_PE + 2]), rb = mk(rw[TR_RB], rw[TR_RB + 1], rw[TR_RB + 2]);
            const float as_e = lane_value((ti < 64) ? vj[1] : vj[2], ti & 63) - dot(pe, al);
            const f3 u = al + cross(aa, rb);                                   // acceleration of the body point under the contact: b_d . aa = (rb x a_d) . aa = a_d . (aa x rb)
            const float f[3] = {rw[TR_F], rw[TR_F + 1], rw[TR_F + 2]};
            float r[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) r[d] = fmaf((d == 0) ? rw[TR_RN] : rw[TR_RN] * (1.0f / IMPRATIO), f[d], rw[TR_RES + d]) + dot(ta[d], u) + rw[TR_C + d] * as_e;
            float fc[3] = {f[0], f[1], f[2]}, lam = rw[TR_LAM];
            float df[3] = {f[0], f[1], f[2]};
            if (!init) {
                visit(rw[TR_BD], rw[TR_BD + 1], rw[TR_BD + 2], rw[TR_BD + 3], rw[TR_BD + 4], rw[TR_BD + 5], r, f, mu_table, lam, fc);
                df[0] = fc[0] - f[0]; df[1] = fc[1] - f[1]; df[2] = fc[2] - f[2];
                *reinterpret_cast<float4*>(&rec[TR_E]) = make_float4(rw[TR_E], fc[0], fc[1], fc[2]);
                rec[TR_LAM] = lam;
            }
            const f3 dgl = ta[0] * df[0] + ta[1] * df[1] + ta[2] * df[2];
            push(dgl, cross(rb, dgl), rw[TR_C] * df[0] + rw[TR_C + 1] * df[1] + rw[TR_C + 2] * df[2], pe, lj[0], lj[1], lj[2]);
        };
        // sweep -1 (warm start only): the running sums take up the forces of the previous step; then pgs_iters sweeps
        for (int it = wst ? -1 : 0; it < C.pgs_iters; ++it) {
            const bool init = it < 0;
            for (int v = 0; v < nc; ++v) probe_visit(v, init);
            // table contacts, software-pipelined by hand: the record of contact i + 1 and its three words of L^-1 are asked for at the top of visit i (a contact's force
            // is changed by its own visit only, so the record cannot go stale), two register sets alternate, and nothing inside the loop waits for memory but the visit
            // that uses it.  (One wave: LDS traffic is served in issue order, so a record written by this visit is what a later visit reads -- no fence.)
            if (ntc > 0) {
                float ra[FTREC], rb_[FTREC], la[3], lb[3];
                load_trec(0, ra, la);
                for (int ti = 0; ti < ntc; ti += 2) {
                    load_trec(ti + 1 < ntc ? ti + 1 : ti, rb_, lb);
                    table_visit(ti, ra, la, init);
                    if (ti + 1 < ntc) {
                        load_trec(ti + 2 < ntc ? ti + 2 : ti + 1, ra, la);
                        table_visit(ti + 1, rb_, lb, init);
                    }
                }
            }
            if (pairB) for (int v = 0; v < nc; ++v) probe_visit(8 + v, init);
        }
    }
    // ---- the next step's warm start: every element's table entry (zeros without a contact), the probe slots ----
    if (wout) {
        group_sync();
#pragma unroll
        for (int i = 0; i < FE; ++i) if (ex[i]) *reinterpret_cast<float4*>(&wout[LATF_WTAB + 4 * (FE * lane + i)]) = make_float4(0.f, 0.f, 0.f, 0.f);
        group_sync();                                                       // (the entries of the contacts are written after the zeros, by other lanes)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int ti = lane + 64 * k;
            if (ti < ntc) {
                const float* rec = &lds[FL_TREC + ti * FTREC];
                *reinterpret_cast<float4*>(&wout[LATF_WTAB + 4 * __float_as_int(rec[TR_E])]) = make_float4(rec[TR_F], rec[TR_F + 1], rec[TR_F + 2], rec[TR_LAM]);
            }
        }
        if (lane < MAXC) wout[LATF_WPROBE + lane] = __int_as_float(lane < nc ? __float_as_int(lds[FL_CAND + 8 * lane + 6]) : -1);
        if (lane < 16) {
            const bool valid = (lane & 7) < nc && (lane < 8 || pairB);
            const float* rec = &lds[FL_REC + lane * FREC];
            *reinterpret_cast<float4*>(&wout[LATF_WPROBE + 8 + 4 * lane]) = valid ? make_float4(rec[FR_F], rec[FR_F + 1], rec[FR_F + 2], rec[FR_LAM]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // ---- accelerations of the contact forces on every element: L y = g_s (scattered by the lanes that built the contacts), a_s = y / m - P a_l ----
    float gs[FE];
    group_sync();
#pragma unroll
    for (int i = 0; i < FE; ++i) lds[FL_U + FE * lane + i] = 0.f;
    group_sync();
    if (nv > 0) {
        // contacts A, contacts B, table contacts one after the other: inside each of the three no element occurs twice
        for (int pass = 0; pass < 2; ++pass) {
            if (lane < 16 && (lane >> 3) == pass && (lane & 7) < nc && (lane < 8 || pairB)) {
                const float* rec = &lds[FL_REC + lane * FREC];
                lds[FL_U + __float_as_int(rec[FR_E])] += rec[FR_C] * rec[FR_F] + rec[FR_C + 1] * rec[FR_F + 1] + rec[FR_C + 2] * rec[FR_F + 2];
            }
            group_sync();
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int ti = lane + 64 * k;
            if (ti < ntc) {
                const float* rec = &lds[FL_TREC + ti * FTREC];
                lds[FL_U + __float_as_int(rec[TR_E])] += rec[TR_C] * rec[TR_F] + rec[TR_C + 1] * rec[TR_F + 1] + rec[TR_C + 2] * rec[TR_F + 2];
            }
        }
        group_sync();
    }
#pragma unroll
    for (int i = 0; i < FE; ++i) gs[i] = lds[FL_U + FE * lane + i];
    float y2[FE];
#pragma unroll
    for (int i = 0; i < FE; ++i) y2[i] = 0.f;
    if (nv > 0) full_cg(lds, lane, nb, dg, M.wten, gs, y2);
#pragma unroll
    for (int i = 0; i < FE; ++i) acc[i] = ex[i] ? at_s[i] + y2[i] * (1.0f / ELEM_MASS) - dot(Pe[i], al) : 0.f;
    ab[0] = at_l.x + al.x; ab[1] = at_l.y + al.y; ab[2] = at_l.z + al.z; ab[3] = aa.x; ab[4] = aa.y; ab[5] = aa.z;
}

