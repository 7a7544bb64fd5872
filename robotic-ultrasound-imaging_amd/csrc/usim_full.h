// usim_full.h -- the FULL torso (usim_config.torso = USIM_TORSO_FULL) as a HIP workload: the rest of SURVEY.md section 8 row a3.  All 270 shell elements of the
// 9 x 4 x 11 composite (soft_box.xml:9) are dynamic sliders on the free torso body that ultrasound.py:426-431 writes at reset; the body rests on the table through
// element-table contacts (ultrasound_arena.py:55-58, friction 1).  One convex problem with the arm, solved in its dual over the probe-element contacts (<= 8 pairs,
// two coincident contacts each) and the element-table contacts (~54 while the box rests) by a block Gauss-Seidel whose visit is the continuous local solve of the top-face
// model's iteration (cone_local), taken in full -- the oracle's full torso (oracle/usim_oracle.c constrained_forward_full / cone_pgs_dense) runs the same model in the same
// order of visits on dense matrices; this file is written independently of it.  The solve starts from the forces of the previous physics step (LATF_WTAB / LATF_WPROBE in the
// environment's lattice block): cold, 24 sweeps over ~54 coupled sticking contacts are nowhere near converged (profiles/r05/full_torso_convergence.txt).
//
// Mapping: ONE WAVE PER ENVIRONMENT (usim_step_kernel<2, 64, MODE>, at the end of this file behind full_forward, as a sequence of named phases: the arm mathematics
// is replicated in the 64 lanes; the torso is what the lanes share).  Lane l owns elements 5 l .. 5 l + 4 (s, sdot in registers).
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
// (included by usim_kernels.hip inside namespace usim, after probe_sdf / group_sync, cone_local of usim_contact.h and usim_episode.h)

// (NSH, FE, FNE, the layout FT_* of a full-torso handle's table block and the layout LATF_* of an environment's lattice block: usim_device.h -- the host reads and writes them)
constexpr int FULL_CG_ITERS = 20;
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
            // cone_local (usim_contact.h), the continuous local solve of the top-face model's iteration, taken in full (Gauss-Seidel: no line search)
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
        for (int half = 0; half < 2; ++half) {
            if (lane < 16 && (lane >> 3) == half && (lane & 7) < nc && (lane < 8 || pairB)) {
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

// ======================================================================================================================================================================
// usim_step_kernel<2, 64, MODE>: the step / reset kernel of the full torso, one workgroup = one wave = one environment (the rigid and soft torsos run usim_step16.h).
// MODE 0: one env.step() per environment; a finished environment takes its next initial state from the reset bank (bank_adopt).
// MODE 1: reset computation (reset_draws, initial_pose_ik, zero-torque forward pass) for the environments selected by the mask (written to the live state) or
//         for the (env, episode) items of the refill work list (written to the reset bank: bank_park).
// full_item is the body of one environment / work item: a sequence of the phases below.  The arm mathematics is the serial chain of usim_devmath.h, replicated in the lanes.
// ======================================================================================================================================================================
constexpr int FULL_NT = 64, FULL_EPB = 1, FULL_LDS_WORDS = FL_WORDS;     // threads and environments per workgroup, dynamic LDS words (full_row, usim_api.hip)

// site Jacobian J = [Jv; Jw]
DI void site_jacobian(const Kin& K, float (&J)[6][NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        f3 jv = cross(K.z[j], K.x - K.o[j]);
        J[0][j] = jv.x; J[1][j] = jv.y; J[2][j] = jv.z; J[3][j] = K.z[j].x; J[4][j] = K.z[j].y; J[5][j] = K.z[j].z;
    }
}
// y = J v
DI void jacobian_mul(const float (&J)[6][NJ], const float* v, float* y) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) s = fmaf(J[a][j], v[j], s);
        y[a] = s;
    }
}
// kinematics, dynamics with the rotor inertias (usim_config.armature_scale), site Jacobian, Cholesky factor of M
DI void arm_dynamics(const DevModel& M, const float* q, const float* qd, Kin& K, Dyn& D, float (&J)[6][NJ], float* Lm, float* idm) {
    fk(M, q, K);
    dynamics(M, K, qd, D);
#pragma unroll
    for (int i = 0; i < NJ; ++i) D.M[PK(i, i)] += M.armature[i];
    site_jacobian(K, J);
#pragma unroll
    for (int k = 0; k < 28; ++k) Lm[k] = D.M[k];
    chol_packed<NJ>(Lm, idm);
}
// Lambda^-1 = J M^-1 J^T = Y^T Y with Y = Lm^-1 J^T (six forward substitutions only; packed lower 6x6)
DI void task_inertia_inv(const float (&J)[6][NJ], const float* Lm, const float* idm, float* Li) {
    float Y[6][NJ];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) Y[a][j] = J[a][j];
        chol_forward<NJ>(Lm, idm, Y[a]);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) s = fmaf(Y[a][j], Y[b][j], s);
            Li[PK(a, b)] = s;
        }
}
// the task's goal frame (columns of M.grot) and the orientation error of the site against a goal frame (osc.py orientation_error)
DI void goal_frame(const DevModel& M, f3& gx, f3& gy, f3& gz) { gx = mk(M.grot[0], M.grot[3], M.grot[6]); gy = mk(M.grot[1], M.grot[4], M.grot[7]); gz = mk(M.grot[2], M.grot[5], M.grot[8]); }
DI f3 orientation_error(const Kin& K, const f3 gx, const f3 gy, const f3 gz) { return (cross(K.sx, gx) + cross(K.sy, gy) + cross(K.sz, gz)) * 0.5f; }

// the environment's scalar words (ten 16-byte loads, Field order) -> joint state and episode scalars; the joint words of the state hold dq = q - q0 (usim_device.h)
DI void state_load(const float* st, const int ei, float* q, float* qd, float* q0, float* dq, Episode& E) {
    float sv[F_NSCALAR];
    const float4* sp = reinterpret_cast<const float4*>(st + scalar_index(0, (size_t)ei));
#pragma unroll
    for (int v = 0; v < F_NSCALAR / 4; ++v) { const float4 x = sp[v]; sv[4 * v] = x.x; sv[4 * v + 1] = x.y; sv[4 * v + 2] = x.z; sv[4 * v + 3] = x.w; }
#pragma unroll
    for (int i = 0; i < NJ; ++i) { dq[i] = sv[F_Q + i]; qd[i] = sv[F_QD + i]; q0[i] = sv[F_Q0 + i]; q[i] = q0[i] + dq[i]; }
    E.ts = mk(sv[F_TS], sv[F_TS + 1], sv[F_TS + 2]); E.te = mk(sv[F_TE], sv[F_TE + 1], sv[F_TE + 2]);
    E.u0 = sv[F_U0]; E.vbar = sv[F_VBAR]; E.fzbar = sv[F_FZBAR]; E.fzprev = sv[F_FZPREV]; E.dfz = sv[F_DFZ];
    E.kst = sv[F_KST]; E.kdmp = sv[F_KDMP]; E.mu = sv[F_MU]; E.epret = sv[F_EPRET];
    E.t = __float_as_int(sv[F_T]); E.touched = __float_as_int(sv[F_TOUCH]); E.episode = __float_as_int(sv[F_EPISODE]); E.status = __float_as_int(sv[F_STATUS]);
}
// 16-byte stores of the quads that hold a changed word (q, qd | running statistics | counters); the quads of per-episode constants only when an episode starts (all)
DI void state_store(float* st, const int ei, const bool all, const float* qd, const float* q0, const float* dq, const Episode& E) {
    float o[F_NSCALAR];
#pragma unroll
    for (int i = 0; i < NJ; ++i) { o[F_Q + i] = dq[i]; o[F_QD + i] = qd[i]; o[F_Q0 + i] = q0[i]; }
    o[F_TS] = E.ts.x; o[F_TS + 1] = E.ts.y; o[F_TS + 2] = E.ts.z; o[F_TE] = E.te.x; o[F_TE + 1] = E.te.y; o[F_TE + 2] = E.te.z;
    o[F_U0] = E.u0; o[F_VBAR] = E.vbar; o[F_FZBAR] = E.fzbar; o[F_FZPREV] = E.fzprev; o[F_DFZ] = E.dfz;
    o[F_KST] = E.kst; o[F_KDMP] = E.kdmp; o[F_MU] = E.mu; o[F_EPRET] = E.epret;
    o[F_T] = __int_as_float(E.t); o[F_TOUCH] = __int_as_float(E.touched); o[F_EPISODE] = __int_as_float(E.episode); o[F_STATUS] = __int_as_float(E.status);
    float4* sp = reinterpret_cast<float4*>(st + scalar_index(0, (size_t)ei));
#pragma unroll
    for (int v = 0; v < F_NSCALAR / 4; ++v) {
        const bool changed = (v <= 3) || v == 7 || v == 8 || v == 9;      // words 0-15 (q, qd, q0[0..1]), 28-31, 32-39
        if (changed || all) sp[v] = make_float4(o[4 * v], o[4 * v + 1], o[4 * v + 2], o[4 * v + 3]);
    }
}

// the free body: spawn pose of a reset (ultrasound.py:426-431), and its 13 words in the environment's lattice block
DI void body_spawn(const DevModel& M, FullBody& b) {
    b.p = mk(M.torso[0], M.torso[1], M.torso[2]); b.q[0] = 1.f; b.q[1] = b.q[2] = b.q[3] = 0.f; b.v = mk(0.f, 0.f, 0.f); b.w = mk(0.f, 0.f, 0.f);
}
DI void body_load(const float* latp, FullBody& b) {
    float bw[13];
#pragma unroll
    for (int a = 0; a < 13; ++a) bw[a] = latp[LATF_BODY + a];
    b.p = mk(bw[0], bw[1], bw[2]); b.q[0] = bw[3]; b.q[1] = bw[4]; b.q[2] = bw[5]; b.q[3] = bw[6];
    b.v = mk(bw[7], bw[8], bw[9]); b.w = mk(bw[10], bw[11], bw[12]);
}
DI void body_store(float* latp, const FullBody& b) {
    const float bw[13] = {b.p.x, b.p.y, b.p.z, b.q[0], b.q[1], b.q[2], b.q[3], b.v.x, b.v.y, b.v.z, b.w.x, b.w.y, b.w.z};
#pragma unroll
    for (int a = 0; a < 13; ++a) latp[LATF_BODY + a] = bw[a];
}
// an episode starts without a warm start of the contact solve (every lane of the wave)
DI void warm_table_clear(float* latp, const int lane) {
    for (int w = lane; w < LATF_WARM_WORDS; w += FULL_NT) latp[LATF_WTAB + w] = (w >= 4 * NSH && w < 4 * NSH + 8) ? __int_as_float(-1) : 0.f;
}

// the action of the step: drawn in the kernel (LF_RANDOM_ACT; same stream as usim_random_actions_kernel) or the caller's
DI void step_action(const DevCfg& C, const DevIO& io, const int flags, const long long rstep, const int ei, const bool store, float* act) {
    if (flags & LF_RANDOM_ACT) {
        uint32_t gid = (uint32_t)(C.env_offset + ei);
        u4 r1 = philox(gid, (uint32_t)rstep, (uint32_t)((unsigned long long)rstep >> 32), 1u, C.key0, C.key1);
        u4 r2 = philox(gid, (uint32_t)rstep, (uint32_t)((unsigned long long)rstep >> 32), 2u, C.key0, C.key1);
        uint32_t rr[8] = {r1.a, r1.b, r1.c, r1.d, r2.a, r2.b, r2.c, r2.d};
#pragma unroll
        for (int a = 0; a < 7; ++a) {
            act[a] = synthetic_action(C, rr[a], a);
            if (io.act_out && store && a < C.adim) io.act_out[(size_t)ei * C.adim + a] = act[a];
        }
    } else {
#pragma unroll
        for (int a = 0; a < 7; ++a) if (a < C.adim) act[a] = finite_or_zero(io.act[(size_t)ei * C.adim + a]);
    }
}

// reset draws of episode ep (ultrasound.py:416-478): trajectory, start point, position noise, solref and friction randomisation -- or the caller's reset_params
DI void reset_draws(const DevModel& M, const DevCfg& C, const DevIO& io, const int ei, const int ep, Episode& E, f3& noise) {
    uint32_t gid = (uint32_t)(C.env_offset + ei);
    u4 A = philox(gid, (uint32_t)ep, 0u, 0u, C.key0, C.key1);
    u4 B = philox(gid, (uint32_t)ep, 1u, 0u, C.key0, C.key1);
    u4 Cc = philox(gid, (uint32_t)ep, 2u, 0u, C.key0, C.key1);
    const float tz = M.torso[2] + M.base[2] + C.top_off;      // ultrasound.py:184,807
    noise = mk(0, 0, 0);
    E.kst = C.stiffness; E.kdmp = C.damping;
    if (io.reset_params) {
        const float* p = io.reset_params + (size_t)ei * 13;
        E.ts = mk(p[0], p[1], p[2]); E.te = mk(p[3], p[4], p[5]); E.u0 = p[6]; noise = mk(p[7], p[8], p[9]);
        E.kst = p[10]; E.kdmp = p[11]; E.mu = p[12];
        return;
    }
    if (C.det_traj) { E.ts = mk(0.062f, -0.020f, 0.896f); E.te = mk(-0.032f, -0.075f, 0.896f); }   // ultrasound.py:763-764
    else {
        // ultrasound.py:787-788: np.linspace grids over the torso top, 50 points each
        const float tx = M.torso[0] + M.base[0], ty = M.torso[1] + M.base[1];
        const float xs = -0.15f + tx + 0.03f, xstep = (0.15f + tx - xs) / 49.f;
        const float ys = -C.y_range + ty, ystep = 2.f * C.y_range / 49.f;
        E.ts = mk(xs + (float)urange(A.a, 50u) * xstep, ys + (float)urange(A.b, 50u) * ystep, tz);
        E.te = mk(xs + (float)urange(A.c, 50u) * xstep, ys + (float)urange(A.d, 50u) * ystep, tz);
    }
    E.u0 = u01(B.a);                                           // ultrasound.py:443
    if (C.rand_pos) {                                        // ultrasound.py:880-881
        float r1 = sqrtf(-2.f * logf(u01_open(B.b))), th1 = 2.f * PI_F * u01(B.c);
        float r2 = sqrtf(-2.f * logf(u01_open(B.d))), th2 = 2.f * PI_F * u01(Cc.a);
        noise = mk(r1 * cosf(th1) * 0.0025f, r1 * sinf(th1) * 0.0025f, r2 * cosf(th2) * 0.010f);
    }
    if (C.rand_solref) { E.kst = 1300.f + (float)urange(Cc.b, 300u); E.kdmp = 17.f + (float)urange(Cc.c, 24u); }   // ultrasound.py:293-294
    float pf = C.probe_fric;
    if (C.rand_fric) pf *= 0.5f + 1.5f * u01(Cc.d);
    E.mu = fmaxf(pf, C.elem_fric);
    if (C.probe_geoms == 2 && !C.pair) E.mu = 0.5f * (E.mu + fmaxf(C.probe_fric2, C.elem_fric));   // two coincident contacts per pair restated as one (usim_config.probe_geoms)
}

// initial pose: damped-least-squares IK from init_qpos to the start point of the trajectory (ultrasound.py:812-844)
DI void initial_pose_ik(const DevModel& M, const DevCfg& C, const Episode& E, const f3 noise, float* q) {
    float uu = clampf(E.u0, 0.f, 1.f);
    f3 tp0 = E.ts + (E.te - E.ts) * uu;
    f3 target = mk(tp0.x + noise.x + M.ikb[0] - M.base[0], tp0.y + noise.y + M.ikb[1] - M.base[1], tp0.z + noise.z + M.ikb[2] - M.base[2]);
#pragma unroll
    for (int i = 0; i < NJ; ++i) q[i] = INITQ[i];
    for (int it = 0; it < C.ik_iters; ++it) {
        Kin K; fk(M, q, K);
        f3 gx, gy, gz; goal_frame(M, gx, gy, gz);
        f3 eo = orientation_error(K, gx, gy, gz);
        f3 ep = target - K.x;
        float e[6] = {ep.x, ep.y, ep.z, eo.x, eo.y, eo.z};
        float J[6][NJ];
        site_jacobian(K, J);
        float A6[21], id6[6];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                float s = (a == b) ? 1e-6f : 0.f;
#pragma unroll
                for (int j = 0; j < NJ; ++j) s = fmaf(J[a][j], J[b][j], s);
                A6[PK(a, b)] = s;
            }
        chol_packed<6>(A6, id6);
        chol_solve<6>(A6, id6, e);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float s = 0.f;
#pragma unroll
            for (int a = 0; a < 6; ++a) s = fmaf(J[a][j], e[a], s);
            q[j] += s;
        }
    }
}

// OSC_POSE torque (robosuite osc.py run_controller; rl_config.yaml:33-51); E.t already counts this step
DI void osc_torque(const DevModel& M, const DevCfg& C, const Episode& E, const float* act, const float inv_h, const Kin& K, const Dyn& D, const float (&J)[6][NJ],
                   const float* Li, const float* q, const float* qd, const float* q0, float* tau) {
    float kp[6], kd[6];
    f3 gpos, gx, gy, gz;
    float up = clampf((float)(E.t - 1) * inv_h + E.u0, 0.f, 1.f);   // controller.traj_pos from the previous _post_action
    f3 tpw = E.ts + (E.te - E.ts) * up;
    if (C.mode == 1) {
        float d[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) d[a] = clampf(act[a], -1.f, 1.f) * (a < 3 ? C.out_pos : C.out_ori);
        gpos = K.x + mk(d[0], d[1], d[2]);
        float ang = sqrt_(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
        if (ang < 1e-12f) { gx = K.sx; gy = K.sy; gz = K.sz; }
        else {
            float hh = 0.5f * ang, sh = sinf(hh) * rcp_(ang), qw = cosf(hh), qx = d[3] * sh, qy = d[4] * sh, qz = d[5] * sh;
            // rotation matrix of the delta quaternion, applied on the left of the current orientation
            f3 e0 = mk(1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy + qw * qz), 2.f * (qx * qz - qw * qy));
            f3 e1 = mk(2.f * (qx * qy - qw * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz + qw * qx));
            f3 e2 = mk(2.f * (qx * qz + qw * qy), 2.f * (qy * qz - qw * qx), 1.f - 2.f * (qx * qx + qy * qy));
            gx = e0 * K.sx.x + e1 * K.sx.y + e2 * K.sx.z;
            gy = e0 * K.sy.x + e1 * K.sy.y + e2 * K.sy.z;
            gz = e0 * K.sz.x + e1 * K.sz.y + e2 * K.sz.z;
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) { kp[a] = C.kp_fixed; kd[a] = 2.f * sqrt_(C.kp_fixed) * C.damping_ratio; }
    } else {
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            float v = (C.mode == 3) ? 0.f : clampf(act[a], 0.f, 1.f);     // wrench mode: no impedance term
            kp[a] = C.kp_min + v * (C.kp_max - C.kp_min);
            kd[a] = 2.f * sqrt_(kp[a]) * C.damping_ratio;
        }
        gpos = mk(tpw.x - M.base[0], tpw.y - M.base[1], tpw.z - M.base[2]);
        if (C.mode == 2) gpos.z += clampf(act[6], -1.f, 1.f) * C.out_pos;
        goal_frame(M, gx, gy, gz);
    }
    float v6[6];
    jacobian_mul(J, qd, v6);
    f3 eo = orientation_error(K, gx, gy, gz);
    f3 ep = gpos - K.x;
    float Fp[3] = {ep.x * kp[0] - v6[0] * kd[0], ep.y * kp[1] - v6[1] * kd[1], ep.z * kp[2] - v6[2] * kd[2]};
    float Tp[3] = {eo.x * kp[3] - v6[3] * kd[3], eo.y * kp[4] - v6[4] * kd[4], eo.z * kp[5] - v6[5] * kd[5]};
    if (C.mode == 3) {
        // fork-only "wrench" baseline (utils/plot.py:267-268; checkpoint action box [-10,10]^6): the action takes the place
        // of desired_force / desired_torque in the OSC law, i.e. wrench = [Lambda_pos a_f; Lambda_ori a_t].  Inferred; the
        // shipped `wrench` policy replayed under this reading earns 9.2 reward/step (8.6 on MuJoCo), under "action =
        // wrench" it fails within 80 steps (tests/test_gpu_policy_replay.py)
#pragma unroll
        for (int a = 0; a < 3; ++a) { Fp[a] = clampf(act[a], -WRENCH_MAX, WRENCH_MAX); Tp[a] = clampf(act[3 + a], -WRENCH_MAX, WRENCH_MAX); }
    }
    // lambda_pos F, lambda_ori T : solves with the 3x3 diagonal blocks of Li (uncouple_pos_ori, rl_config.yaml:48)
    {
        float P3[6] = {Li[PK(0, 0)], Li[PK(1, 0)], Li[PK(1, 1)], Li[PK(2, 0)], Li[PK(2, 1)], Li[PK(2, 2)]}, ip[3];
        chol_packed<3>(P3, ip); chol_solve<3>(P3, ip, Fp);
        float O3[6] = {Li[PK(3, 3)], Li[PK(4, 3)], Li[PK(4, 4)], Li[PK(5, 3)], Li[PK(5, 4)], Li[PK(5, 5)]}, io3[3];
        chol_packed<3>(O3, io3); chol_solve<3>(O3, io3, Tp);
    }
    float wr[6] = {Fp[0], Fp[1], Fp[2], Tp[0], Tp[1], Tp[2]};
    // nullspace torque N^T M (10 (q0 - q) - 2 sqrt(10) qd)
    float pt[NJ], y[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) pt[i] = 10.f * (q0[i] - q[i]) - 6.3245553203367586f * qd[i];
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) s = fmaf((i >= j) ? D.M[PK(i, j)] : D.M[PK(j, i)], pt[j], s);
        y[i] = s;
    }
    float jb[6];
    jacobian_mul(J, pt, jb);                                  // (M^-1 J^T)^T (M pt) = J pt
    {
        float L6[21], i6[6];
#pragma unroll
        for (int k = 0; k < 21; ++k) L6[k] = Li[k];
        chol_packed<6>(L6, i6); chol_solve<6>(L6, i6, jb);
    }
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        float s = D.bias[i] + y[i];
#pragma unroll
        for (int a = 0; a < 6; ++a) s = fmaf(J[a][i], wr[a] - jb[a], s);
        tau[i] = clampf(s, -TAUMAX[i], TAUMAX[i]);
    }
}

// smooth acceleration of the arm: M^-1 (tau - bias - joint damping), joint friction
DI void smooth_acceleration(const DevCfg& C, const Dyn& D, const float* Lm, const float* idm, const float* tau, const float* qd, float* qs) {
#pragma unroll
    for (int i = 0; i < NJ; ++i) qs[i] = tau[i] - D.bias[i] - JOINT_DAMP * qd[i];
    chol_solve<NJ>(Lm, idm, qs);
    joint_friction(D.M, Lm, idm, qd, C.frictionloss, qs);
}
// constrained arm acceleration: qacc = qs + M^-1 J^T W
DI void constrained_acceleration(const float (&J)[6][NJ], const float* Lm, const float* idm, const float* qs, const float* W, float* qacc) {
    float z[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        float s = 0.f;
#pragma unroll
        for (int a = 0; a < 6; ++a) s = fmaf(J[a][i], W[a], s);
        z[i] = s;
    }
    chol_solve<NJ>(Lm, idm, z);
#pragma unroll
    for (int i = 0; i < NJ; ++i) qacc[i] = qs[i] + z[i];
}

// semi-implicit Euler of the lane's sliders (a reset pass leaves the lattice at rest), stored when `write`; returns the lane's share of the guard sum
template <int MODE>
DI float slider_euler(float* latp, const int lane, const bool write, const float dt, const float (&acc)[FE], const float (&s)[FE], const float (&sd)[FE]) {
    float lat_chk = 0.f;
#pragma unroll
    for (int i = 0; i < FE; ++i) {
        const int e = FE * lane + i;
        float sdn = 0.f, sn = 0.f;
        if (MODE == 0) { sdn = fmaf(dt, acc[i], sd[i]); sn = fmaf(dt, sdn, s[i]); }
        if (write && e < NSH) { latp[LATF_SD + e] = sdn; latp[LATF_S + e] = sn; }
        if (e < NSH) lat_chk += fabsf(sn) + 1e-3f * fabsf(sdn);
    }
    return lat_chk;
}
// semi-implicit Euler of the free body (linear part in world axes, angular velocity in the body frame, quaternion by the exponential of dt w / 2).  Returns what the
// numerical fault guard sees of the torso: the free body's 13 words and every slider (lat_chk: slider_euler) -- a non-finite word makes the sum non-finite; without
// this a torso gone NaN fails every comparison of full_forward, its contacts vanish silently and the arm -- all the guard used to look at -- stays finite
DI float body_euler(FullBody& body, const float* ab, const float dt, const float lat_chk) {
    const float qw = body.q[0], qx = body.q[1], qy = body.q[2], qz = body.q[3];
    const f3 abl = mk(ab[0], ab[1], ab[2]);
    const f3 aw = mk((1.f - 2.f * (qy * qy + qz * qz)) * abl.x + 2.f * (qx * qy - qw * qz) * abl.y + 2.f * (qx * qz + qw * qy) * abl.z,
                     2.f * (qx * qy + qw * qz) * abl.x + (1.f - 2.f * (qx * qx + qz * qz)) * abl.y + 2.f * (qy * qz - qw * qx) * abl.z,
                     2.f * (qx * qz - qw * qy) * abl.x + 2.f * (qy * qz + qw * qx) * abl.y + (1.f - 2.f * (qx * qx + qy * qy)) * abl.z);
    body.v = madd(body.v, aw, dt); body.p = madd(body.p, body.v, dt);
    body.w = madd(body.w, mk(ab[3], ab[4], ab[5]), dt);
    const float wn = sqrt_(dot(body.w, body.w)), hh = 0.5f * dt * wn;
    float shh, chh; sincosf(hh, &shh, &chh);
    const float sh = (wn > 1e-12f) ? shh * rcp_(wn) : 0.5f * dt;
    const float dx = body.w.x * sh, dy = body.w.y * sh, dz2 = body.w.z * sh;
    const float n0 = qw * chh - qx * dx - qy * dy - qz * dz2, n1 = qw * dx + qx * chh + qy * dz2 - qz * dy;
    const float n2 = qw * dy - qx * dz2 + qy * chh + qz * dx, n3 = qw * dz2 + qx * dy - qy * dx + qz * chh;
    const float irn = rsq_(n0 * n0 + n1 * n1 + n2 * n2 + n3 * n3);
    body.q[0] = n0 * irn; body.q[1] = n1 * irn; body.q[2] = n2 * irn; body.q[3] = n3 * irn;
    return wave_sum(lat_chk) + fabsf(body.p.x) + fabsf(body.p.y) + fabsf(body.p.z) + fabsf(body.q[0]) + fabsf(body.q[1]) + fabsf(body.q[2]) + fabsf(body.q[3])
         + 1e-3f * (fabsf(body.v.x) + fabsf(body.v.y) + fabsf(body.v.z) + fabsf(body.w.x) + fabsf(body.w.y) + fabsf(body.w.z));
}

// torque sensor at ft_frame (MuJoCo cfrc_int of the probe body, site frame)
DI void torque_sensor(const DevModel& M, const Kin& K, const Dyn& D, const float (&J)[6][NJ], const float* qacc, const float* W, float* tq) {
    // link-7 accelerations from the site Jacobian: alpha = alpha_bias + Jw qacc, a(o7) = a_bias + Jv qacc - (Jw qacc) x (x - o7)
    float aq[6];
    jacobian_mul(J, qacc, aq);
    const f3 alq = mk(aq[3], aq[4], aq[5]);
    f3 al = D.al7 + alq;
    f3 a7 = D.a7 + mk(aq[0], aq[1], aq[2]) - cross(alq, K.x - K.o[NJ - 1]);
    f3 rc = K.r7x * M.pcom7[0] + K.r7y * M.pcom7[1] + K.r7z * M.pcom7[2];
    f3 ac = a7 + cross(al, rc) + cross(D.w7, cross(D.w7, rc));
    f3 N = rot_inertia_mul(K, M.pI7, al) + cross(D.w7, rot_inertia_mul(K, M.pI7, D.w7));
    f3 Fp = ac * PROBE_MASS;
    f3 tw = N + cross(K.o[NJ - 1] + rc - K.x, Fp) - mk(W[3], W[4], W[5]);
    tq[0] = dot(K.sx, tw); tq[1] = dot(K.sy, tw); tq[2] = dot(K.sz, tw);
}

// integrate the arm: mj_Euler with implicit joint damping.  Returns the hand velocity: Jacobian from before the integration, qvel from after (mj_step data semantics)
DI f3 arm_euler(const Kin& K, const float (&J)[6][NJ], const float* Lm, const float* idm, const float dt, const float* qacc, float* q, float* qd, const float* q0, float* dq) {
    // (M + h D) x = M qacc with D = d I, h d = 2e-5: x = qacc - h d M^-1 x.  One step from x = qacc reuses the factor of M; the
    // contraction is h d / lambda_min(M) = 2.8e-4 (lambda_min(M) = 0.071 kg m^2 over the workspace), so the remainder
    // is 8e-8 relative -- fp32 rounding.  No second factorisation, and the mass matrix is dead before the contact phase.
    float rhs[NJ];
    {
        const float hd = dt * JOINT_DAMP;
        float xk[NJ];
#pragma unroll
        for (int i = 0; i < NJ; ++i) xk[i] = qacc[i];
        chol_solve<NJ>(Lm, idm, xk);
#pragma unroll
        for (int i = 0; i < NJ; ++i) rhs[i] = fmaf(-hd, xk[i], qacc[i]);
    }
#pragma unroll
    for (int i = 0; i < NJ; ++i) { qd[i] = fmaf(dt, rhs[i], qd[i]); dq[i] = fmaf(dt, qd[i], dq[i]); q[i] = q0[i] + dq[i]; }
    float vs2[6];
    jacobian_mul(J, qd, vs2);
    return mk(vs2[0], vs2[1], vs2[2]) + cross(mk(vs2[3], vs2[4], vs2[5]), K.hand - K.x);
}

// observation (ultrasound.py:363-401) at trajectory step tprev; also leaves the site position in world axes, the trajectory point and the site quaternion (xyzw)
DI void observation(const DevModel& M, const Episode& E, const Kin& K, const float* W, const float* tq, const f3 hv, const int tprev, const float inv_h,
                    float* obs, f3& xw, f3& tpw, float* qe) {
    float up = clampf((float)tprev * inv_h + E.u0, 0.f, 1.f);
    tpw = E.ts + (E.te - E.ts) * up;
    obs[0] = W[0]; obs[1] = W[1]; obs[2] = W[2];              // net contact force on the probe (cfrc_ext[probe][3:6])
    obs[3] = tq[0]; obs[4] = tq[1]; obs[5] = tq[2];
    obs[6] = hv.x; obs[7] = hv.y; obs[8] = hv.z;
    obs[9] = E.fzbar - 5.0f; obs[10] = E.dfz - 0.0f; obs[11] = E.vbar - 0.04f;
    xw = mk(K.x.x + M.base[0], K.x.y + M.base[1], K.x.z + M.base[2]);
    obs[12] = xw.x - tpw.x; obs[13] = xw.y - tpw.y; obs[14] = xw.z - tpw.z;
    mat2quat_xyzw(K.sx, K.sy, K.sz, qe);
    difference_quat(qe, M.gquat, obs + 15);               // xyzw arrays through the wxyz routine (ultrasound.py:390)
}

// reward terms of a step, kept for the episode record
struct RewardTerms { float pos, ori, vel, force, dforce, ori_err; bool contact; };
// reward (ultrasound.py:230-269), bookkeeping (:528-546), termination (:635-670) and the numerical fault guard.  Returns the reward.
DI float reward_and_bookkeeping(const DevModel& M, const DevCfg& C, Episode& E, const float* q, const float* qd, const f3 xw, const f3 tpw, const float* qe, const f3 hv,
                                const float fz, const int ncon, const int overflow, const float full_chk, RewardTerms& T, bool& done) {
    T.contact = ncon > 0;
    if (T.contact) E.touched = 1;
    float pe0 = 90.f * (xw.x - tpw.x), pe1 = 90.f * (xw.y - tpw.y);
    pe0 *= pe0; pe1 *= pe1;
    const float pos_err_norm = sqrt_(pe0 * pe0 + pe1 * pe1);
    T.pos = 5.f * exp_(-pos_err_norm);
    float qc[4] = {qe[3], qe[0], qe[1], qe[2]};
    T.ori_err = 0.2f * distance_quat_goal(qc, M.ghat, M.geps);
    T.ori = exp_(-T.ori_err);
    float ve = 45.f * (E.vbar - 0.04f); ve *= ve;
    T.vel = exp_(-ve);
    float fe = 0.7f * (E.fzbar - 5.f); fe *= fe;
    T.force = T.contact ? 3.f * exp_(-fe) : 0.f;
    float de = 0.01f * E.dfz; de *= de;
    T.dforce = T.contact ? 2.f * exp_(-de) : 0.f;
    float reward = T.pos + T.ori + T.vel + T.force + T.dforce;
    done = E.t >= C.horizon;
    float hvn = sqrt_(dot(hv, hv));
    E.vbar += (hvn - E.vbar) * rcp_((float)E.t);
    E.dfz = (fz - E.fzprev) * rcp_(C.dt_ctrl);                 // ultrasound.py:542: self.control_timestep
    E.fzprev = fz;
    E.fzbar = 0.1f * fz + 0.9f * E.fzbar;
    if (C.early_term) {
        bool term = false;
#pragma unroll
        for (int i = 0; i < NJ; ++i) term = term || (q[i] < QMIN[i] + 0.1f) || (q[i] > QMAX[i] - 0.1f);
        term = term || (pos_err_norm > 1.0f) || (T.contact && T.ori_err > 0.10f) || (E.touched && !T.contact);
        done = done || term;
    }
    E.epret += reward;
    if (overflow) E.status |= overflow & 3;                            // (bit 1: more element-table contacts than the kernel keeps)
    // a non-finite or run-away state ends the episode and is flagged
    float chk = full_chk;
#pragma unroll
    for (int i = 0; i < NJ; ++i) chk += fabsf(q[i]) + 1e-3f * fabsf(qd[i]);
    if (!(chk < 1.0e3f)) { E.status |= 4; done = true; E.epret -= reward; reward = 0.f; if (!(E.epret == E.epret)) E.epret = 0.f; }
    return reward;
}

// per-step episode record L in the order of the reference's CSV dump (ultrasound.py:552-614).  The torque and action channels leave the registers right
// after the controller (episode_record_controls) instead of living to the end of the step.
DI void episode_record_controls(float* L, const float* tau, const float* act) {
#pragma unroll
    for (int i = 0; i < NJ; ++i) L[33 + i] = tau[i];
#pragma unroll
    for (int a = 0; a < 7; ++a) L[46 + a] = act[a];
}
DI void episode_record(float* L, const DevModel& M, const Episode& E, const float* q, const f3 xw, const float* qe, const f3 hv, const float fz, const float inv_h, const RewardTerms& T) {
    const float upn = clampf((float)E.t * inv_h + E.u0, 0.f, 1.f);
    const f3 tpn = E.ts + (E.te - E.ts) * upn;                                    // trajectory point after this step's update (:532)
    L[0] = xw.x; L[1] = xw.y; L[2] = xw.z; L[3] = tpn.x; L[4] = tpn.y; L[5] = tpn.z;
    L[6] = hv.x; L[7] = hv.y; L[8] = hv.z; L[9] = 0.04f; L[10] = E.vbar;
    L[11] = qe[0]; L[12] = qe[1]; L[13] = qe[2]; L[14] = qe[3];
    L[15] = M.gquat[0]; L[16] = M.gquat[1]; L[17] = M.gquat[2]; L[18] = M.gquat[3];
    L[19] = T.ori_err * 5.0f;                                                 // distance_quat (ori_err = 0.2 * distance)
    L[20] = fz; L[21] = 5.0f; L[22] = E.fzbar; L[23] = E.dfz; L[24] = 0.f; L[25] = T.contact ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < NJ; ++i) L[26 + i] = q[i];
    L[40] = (float)(E.t - 1) * inv_h * 100.f;
    L[41] = T.pos; L[42] = T.ori; L[43] = T.vel; L[44] = T.force; L[45] = T.dforce;
}
// what a step hands back per environment: reward, status, done, contact list; for a finished episode its last observation, return and length
DI void step_outputs(const DevIO& io, const int ei, const Episode& E, const float reward, const bool done, const int ncon, const int* con_el, const float* obs) {
    io.rew[ei] = reward;
    if (io.status_out) io.status_out[ei] = E.status;
    io.done[ei] = done ? 1 : 0;
    if (io.contacts) {
        io.contacts[(size_t)ei * (1 + MAXC)] = ncon;
#pragma unroll
        for (int k = 0; k < MAXC; ++k) io.contacts[(size_t)ei * (1 + MAXC) + 1 + k] = con_el[k];
    }
    if (done) {
        if (io.term_obs) {
#pragma unroll
            for (int a = 0; a < OBS_DIM; ++a) io.term_obs[(size_t)ei * OBS_DIM + a] = obs[a];
        }
        if (io.ep_ret) io.ep_ret[ei] = E.epret;
        if (io.ep_len) io.ep_len[ei] = E.t;
    }
}
DI void obs_store(const DevIO& io, const int ei, const float* obs) {
#pragma unroll
    for (int a = 0; a < OBS_DIM; ++a) io.obs[(size_t)ei * OBS_DIM + a] = obs[a];
}

// reset computed ahead of time: park it in the bank slot of episode ep (one lane)
DI void bank_park(float* st, const DevIO& io, const int npad, const int ei, const int ep, const float* q, const Episode& E, const float* obs, const int overflow) {
    const int sl = ep & (BANK_DEPTH - 1);
#pragma unroll
    for (int i = 0; i < NJ; ++i) BK(sl, BQ0 + i) = q[i];
    BK(sl, BTS) = E.ts.x; BK(sl, BTS + 1) = E.ts.y; BK(sl, BTS + 2) = E.ts.z; BK(sl, BTE) = E.te.x; BK(sl, BTE + 1) = E.te.y; BK(sl, BTE + 2) = E.te.z;
    BK(sl, BU0) = E.u0; BK(sl, BKST) = E.kst; BK(sl, BKDMP) = E.kdmp; BK(sl, BMU) = E.mu; BK(sl, BFZ) = E.fzbar;
#pragma unroll
    for (int a = 0; a < OBS_DIM; ++a) BK(sl, BOBS + a) = obs[a];
    BKI(sl, BSTATUS) = overflow & 3;
}
// auto-reset: adopt the initial state prepared in the reset bank (SB3 VecEnv semantics: the observation returned for a finished environment is its reset
// observation), put the torso back to its spawn state and queue the slot for refill (every lane of the wave)
DI void bank_adopt(const DevModel& M, float* st, const DevIO& io, const int npad, const int env, const int ei, const int lane, const bool valid, float* latp,
                   float* q, float* qd, float* q0, float* dq, Episode& E) {
    const bool store = valid && lane == 0;
    E.episode += 1;
    const int sl = E.episode & (BANK_DEPTH - 1);
#pragma unroll
    for (int i = 0; i < NJ; ++i) { q[i] = BK(sl, BQ0 + i); q0[i] = q[i]; qd[i] = 0.f; dq[i] = 0.f; }
    E.ts = mk(BK(sl, BTS), BK(sl, BTS + 1), BK(sl, BTS + 2)); E.te = mk(BK(sl, BTE), BK(sl, BTE + 1), BK(sl, BTE + 2));
    E.u0 = BK(sl, BU0); E.kst = BK(sl, BKST); E.kdmp = BK(sl, BKDMP); E.mu = BK(sl, BMU); E.fzbar = BK(sl, BFZ);
    episode_begin(E, BKI(sl, BSTATUS));
    if (store && io.obs) {
#pragma unroll
        for (int a = 0; a < OBS_DIM; ++a) io.obs[(size_t)ei * OBS_DIM + a] = BK(sl, BOBS + a);
    }
    if (valid) {
        // (every word by the lane that wrote it in the step above)
        for (int i = 0; i < FE; ++i) { const int e = FE * lane + i; if (e < NSH) { latp[LATF_S + e] = 0.f; latp[LATF_SD + e] = 0.f; } }
        if (lane == 0) { FullBody b; body_spawn(M, b); body_store(latp, b); }
        group_sync();                                                    // (the step above left its warm start through other lanes)
        warm_table_clear(latp, lane);
    }
    if (store) order_refill(io, env, E.episode);
}

// one environment (MODE 0; MODE 1 with a mask) or one item of the refill work list
template <int MODE>
DI void full_item(float* lds, const DevModel& M, const DevCfg& C, float* __restrict__ st, const int n, const int npad, const DevIO& io, const int flags, const long long rstep,
                  const bool refill, const int item, const int item_cnt) {
    const int lane = threadIdx.x;
    int env = blockIdx.x, item_ep = 0;
    bool valid = env < n;                             // lattice rows are stored by every lane of the wave
    if (refill) {
        valid = item < item_cnt;
        const int2 it = valid ? io.items[item] : make_int2(0, 0);
        env = it.x; item_ep = it.y;
    }
    const bool store = valid && lane == 0;            // per-environment scalars and outputs by its first lane
    const int ei = valid ? env : (refill ? 0 : n - 1);               // clamp so that every lane has something to read; stores are guarded
    float* const latp = st + (size_t)F_LAT * npad + (size_t)ei * LATF_ENV_WORDS;     // the environment's block of the lattice region
    USIM_STAMP(io.dbg, 0);
    float q[NJ], qd[NJ], q0[NJ], dq[NJ];
    Episode E;
    state_load(st, ei, q, qd, q0, dq, E);
    // sliders of this lane (lane l owns elements 5 l .. 5 l + 4): prefetched now, consumed after the arm phase
    float s_pre[FE], sd_pre[FE];
#pragma unroll
    for (int i = 0; i < FE; ++i) {
        const int e = FE * lane + i;
        s_pre[i] = 0.f; sd_pre[i] = 0.f;
        if (MODE == 0 && e < NSH) { s_pre[i] = latp[LATF_S + e]; sd_pre[i] = latp[LATF_SD + e]; }
    }
    FullBody body;
    body_spawn(M, body);
    if constexpr (MODE == 0) body_load(latp, body);
    USIM_STAMP(io.dbg, 1);
    float act[7] = {0, 0, 0, 0, 0, 0, 0};
    if constexpr (MODE == 0) step_action(C, io, flags, rstep, ei, store, act);

    // MODE 1: this item is (re)initialised; MODE 0: the episode ended and the next one is adopted from the bank
    bool need = false;
    const float dt = C.dt, inv_h = rcp_((float)C.horizon);
    int ep_t = E.episode;                             // episode index the reset draws are keyed on
    if constexpr (MODE == 1) {
        need = refill ? valid : (io.mask ? io.mask[ei] != 0 : true);
        if (!__any(need)) return;
        if (need) {
            ep_t = refill ? item_ep : E.episode + 1;                 // listed bank episode, or the live reset
            if (!refill) E.episode = ep_t;
            f3 noise;
            reset_draws(M, C, io, ei, ep_t, E, noise);
            initial_pose_ik(M, C, E, noise, q);
#pragma unroll
            for (int i = 0; i < NJ; ++i) { q0[i] = q[i]; qd[i] = 0.f; dq[i] = 0.f; }
            episode_begin(E, 0);
        }
    } else {
        E.t += 1;                                                    // MujocoEnv.step: timestep += 1
    }

    // forward pass at (q, qd): kinematics, dynamics, controller, constrained accelerations, sensors; then integration and the env logic
    if (MODE == 0 || need) {
        Kin K; Dyn D;
        float J[6][NJ], Lm[28], idm[NJ], Li[21];
        arm_dynamics(M, q, qd, K, D, J, Lm, idm);
        task_inertia_inv(J, Lm, idm, Li);
        USIM_STAMP(io.dbg, 2);
        float tau[NJ];
        if constexpr (MODE == 0) {
            osc_torque(M, C, E, act, inv_h, K, D, J, Li, q, qd, q0, tau);
            if (store && io.log) episode_record_controls(io.log + (size_t)ei * LOG_WIDTH, tau, act);
        } else {
#pragma unroll
            for (int i = 0; i < NJ; ++i) tau[i] = 0.f;      // reset: sim.forward() with zero ctrl
        }
        USIM_STAMP(io.dbg, 3);
        float qs[NJ];
        smooth_acceleration(C, D, Lm, idm, tau, qd, qs);

        // torso (full_forward): 270 sliders on the free body, probe and table contacts.  The contact solve starts from the forces of the previous physics step, kept
        // in the environment's lattice block; a reset pass starts cold and leaves none
        float W[6] = {0, 0, 0, 0, 0, 0};          // site-space wrench of the contact forces
        float alpha[6], vs[6], acc_e[FE], ab[6];
        int cel[MAXC], nc = 0, ovf = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            float s = 0.f, u = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) { s = fmaf(J[a][j], qs[j], s); u = fmaf(J[a][j], qd[j], u); }
            alpha[a] = s; vs[a] = u;
        }
        full_forward(lds, lane, M, C, E.kst, E.kdmp, E.mu, s_pre, sd_pre, body, K.x, K.sx, K.sy, K.sz, Li, alpha, vs, W, acc_e, ab, nc, cel, ovf,
                     (MODE == 0) ? latp : nullptr, (MODE == 0 && valid) ? latp : nullptr);
        // The arm quantities the rest of the pass needs (kinematics, mass matrix and its factor, bias, site Jacobian: ~250 words) are formed AGAIN here, from joint
        // state the compiler cannot recognise, instead of living through the contact solve: 2.5 k instructions against the solve's 700 k, and the kernel is held to 256
        // registers -- two environments per SIMD -- though not cleanly: 141 spilled vector registers and 576 B of scratch per lane in MODE 0, 190 and 556 B in MODE 1
        // (profiles/full_kernel/resource_usage.txt).  Same inputs, same instructions: the same bits.
#pragma unroll
        for (int i = 0; i < NJ; ++i) asm volatile("" : "+v"(q[i]), "+v"(qd[i]));
        arm_dynamics(M, q, qd, K, D, J, Lm, idm);
        const float lat_chk = slider_euler<MODE>(latp, lane, valid && (MODE == 0 || !refill), dt, acc_e, s_pre, sd_pre);
        float full_chk = 0.f;                     // |free body| + sum |sliders| after the integration, for the numerical fault guard
        if constexpr (MODE == 0) full_chk = body_euler(body, ab, dt, lat_chk);
        if (store && (MODE == 0 || !refill)) body_store(latp, body);
        if (MODE == 1 && valid && !refill) warm_table_clear(latp, lane);     // a reset of the live state
        USIM_STAMP(io.dbg, 12);
        float qacc[NJ], tq[3];
        constrained_acceleration(J, Lm, idm, qs, W, qacc);
        torque_sensor(M, K, D, J, qacc, W, tq);
        USIM_STAMP(io.dbg, 13);
        f3 hv = mk(0, 0, 0);
        if constexpr (MODE == 0) hv = arm_euler(K, J, Lm, idm, dt, qacc, q, qd, q0, dq);
        USIM_STAMP(io.dbg, 14);
        if constexpr (MODE == 1) E.fzbar = W[2];                     // ultrasound.py:477
        float obs[OBS_DIM], qe[4];
        f3 xw, tpw;
        observation(M, E, K, W, tq, hv, (MODE == 0) ? E.t - 1 : 0, inv_h, obs, xw, tpw, qe);
        if constexpr (MODE == 0) {
            RewardTerms T;
            bool done;
            const float reward = reward_and_bookkeeping(M, C, E, q, qd, xw, tpw, qe, hv, W[2], nc, ovf, full_chk, T, done);
            if (store && io.log) episode_record(io.log + (size_t)ei * LOG_WIDTH, M, E, q, xw, qe, hv, W[2], inv_h, T);
            if (store) step_outputs(io, ei, E, reward, done, nc, cel, obs);
            need = done && (flags & LF_AUTO_RESET) != 0;
            if (store && io.obs && !need) obs_store(io, ei, obs);
        } else {
            if (refill) { if (store) bank_park(st, io, npad, ei, ep_t, q, E, obs, ovf); }
            else if (store && io.obs) obs_store(io, ei, obs);
            if (ovf) E.status |= ovf & 3;
        }
    }
    if (MODE == 0 && need) bank_adopt(M, st, io, npad, env, ei, lane, valid, latp, q, qd, q0, dq, E);
    USIM_STAMP(io.dbg, 15);
    if (store && !(MODE == 1 && (refill || !need))) state_store(st, ei, (MODE == 1) || need, qd, q0, dq, E);
}

template <int TORSO, int G, int MODE>
__global__ __launch_bounds__(FULL_NT, 2) void usim_step_kernel(const DevModel M, const DevCfg C, float* __restrict__ st, int n, int npad, const DevIO io, int flags, long long rstep) {
    static_assert(TORSO == 2 && G == FULL_NT && FULL_EPB == 1, "the full torso's mapping only: one wave per environment");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // step waves outrank the background refill waves that may share their SIMD (priority, then age, arbitrates VALU issue)
    __builtin_amdgcn_s_setprio(MODE == 0 ? 3 : 0);
    // refill launches walk the work list with a grid-stride loop; every other launch runs the body once
    const bool refill = (MODE == 1) && io.refill != 0;
    const int item_cnt = refill ? io.count[0] : 1;
    for (int item = refill ? (int)blockIdx.x : 0; item < item_cnt; item += refill ? (int)gridDim.x : 1) {
        full_item<MODE>(lds, M, C, st, n, npad, io, flags, rstep, refill, item, item_cnt);
        if (refill) group_sync();                     // the next item reuses the LDS block
    }
    if (MODE == 1 && refill) work_list_close(io);
    USIM_STAMP(io.dbg, 16);
}
