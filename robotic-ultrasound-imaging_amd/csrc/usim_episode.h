// usim_episode.h -- per-environment pieces of what the reference's Ultrasound env does around mj_step.  The Episode struct, the reset-bank
// addressing, episode_begin, order_refill, work_list_close and finite_or_zero serve the step kernel of the full torso (usim_full.h) and the
// 16-lane kernels of the rigid and soft torsos (usim_step16.h); synthetic_action serves the full-torso kernel and usim_random_actions_kernel.
// The functions work on per-environment scalars; what is laid out per lane (joint words, the Philox evaluation) stays with the kernels.
// Still one copy per kernel family: reset draws, observation, reward terms, bookkeeping, termination, episode record, bank park / adopt, and
// (in step16_one, the pass of the single-wave 16-lane kernels and of the split kernel's arm wave; its lattice wave, lattice_pass, has none of these) the synthetic-action
// decoding.  Moved into force-inlined functions they compute the same values, but the 16-lane kernels come
// out with a different instruction schedule and register allocation (the callee is simplified on its own before it is inlined; synthetic_action
// in step16_one changes 7 of the 14), which needs an A/B of its own.
#pragma once
// (included by usim_kernels.hip inside namespace usim, after usim_contact.h, before usim_full.h)

// the per-episode scalar words of the state (Field F_TS .. F_STATUS)
struct Episode {
    f3 ts, te;
    float u0, vbar, fzbar, fzprev, dfz, kst, kdmp, mu, epret;
    int t, touched, episode, status;
};

// word f of the reset-bank slot `slot` (BankField; BKI: as int) of the environment, in the step kernels: st, io, npad and ei are theirs
#define USIM_BANK_INDEX(slot, f) ((size_t)io.bank_row0 * npad + ((size_t)ei * BANK_DEPTH + (slot)) * BANK_STRIDE + (f))
#define BK(slot, f) st[USIM_BANK_INDEX(slot, f)]
#define BKI(slot, f) (reinterpret_cast<int*>(st))[USIM_BANK_INDEX(slot, f)]

// counters of a new episode (status: the reset's own bits)
DI void episode_begin(Episode& E, const int status) {
    E.t = 0; E.touched = 0; E.fzprev = 0.f; E.dfz = 0.f; E.vbar = 0.f; E.epret = 0.f; E.status = status;
}

// auto-reset consumed the bank slot of `episode`: order the episode that will occupy it (computed by the next bulk refill, which runs at least
// every BANK_DEPTH steps, i.e. before this environment can come round to the slot again)
DI void order_refill(const DevIO& io, const int env, const int episode) {
    const int idx = atomicAdd(io.count, 1);
    io.items[idx] = make_int2(env, episode + BANK_DEPTH);
}

// end of a refill launch: the last workgroup to finish empties the work list for the step kernels that follow on the stream
DI void work_list_close(const DevIO& io) {
    __syncthreads();
    if (threadIdx.x == 0) {
        // (no device-scope fence: the list is read by the launches that FOLLOW on the stream, and a fence costs an L2 write-back per wave)
        if (atomicAdd(io.count + 1, 1) == (int)gridDim.x - 1) { io.count[0] = 0; io.count[1] = 0; }
    }
}

// component a of the synthetic action of BASELINE.md section 4 from the Philox word r
DI float synthetic_action(const DevCfg& C, const uint32_t r, const int a) {
    const float u = u01(r);
    const bool sgn = (C.mode == 1) || (C.mode == 3) || (C.mode == 2 && a == 6);
    const float v = sgn ? 2.f * u - 1.f : u;
    return (C.mode == 3) ? v * WRENCH_MAX : v;
}

// a non-finite component of a policy action is treated as 0
DI float finite_or_zero(const float v) { return (v == v && fabsf(v) <= 3.0e38f) ? v : 0.f; }
