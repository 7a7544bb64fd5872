"""The population kernels (csrc/usim_policy.hip: usim_policy_pack_multi / usim_policy_step_multi / usim_policy_reward_multi) through their C ABI against their
contract: a call computes, bit for bit, what K calls of the single-network entry point compute on the slices -- every output word, every word of the statistics,
and the guard words behind the outputs.  Members carry distinct random weights and distinct non-trivial statistics.  (K, G): one workgroup per member, a one-row
tail, two full workgroups plus a tail, a member smaller than a wave.  The comparisons are torch.equal on the words' integer views; there is no tolerance."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 32), (3, 32), (3, 33), (2, 70), (5, 1)]
ADIMS = [6, 7]
GUARD = 64
SENTINEL = -7.25e33
SEED, COUNTER, CTR_BASE, ENV_OFFSET = 0x123456789ABC, 3, 11, 1000
STAT_NAMES = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "returns", "scratch")
OUT_NAMES = ("act_env", "nobs", "act", "value", "logp", "start")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32).reshape(-1)


class Case:
    """K members x G environments: parameters [K][stride], K-major statistics, one observation / done / reward batch -- built once per (K, G, A), never modified
    (every run works on clones)"""

    def __init__(self, usim, K, G, A):
        L = usim._lib
        self.usim, self.lib, self.K, self.G, self.A, self.n = usim, L.load(), K, G, A, K * G
        g = torch.Generator().manual_seed(1000 * K + 10 * G + A)
        r = lambda *s: torch.randn(*s, generator=g)
        self.P = usim.learner.ppo_params(A)
        self.stride = (self.P + 3) // 4 * 4 + 4                        # (a row longer than it needs to be: the words behind P are never read)
        self.sizes = [math.prod(s) for s in usim.learner._field_shapes(A)]
        theta = torch.full((K, self.stride), float("nan"))             # ... and hold NaN here
        for k in range(K):
            o = 0
            for (name, _), size in zip(usim.learner.FIELDS, self.sizes):
                scale = {"pi_w1": 0.4, "vf_w1": 0.4, "pi_w2": 0.12, "vf_w2": 0.12, "act_w": 0.2, "val_w": 0.2}.get(name, 0.3)
                theta[k, o:o + size] = scale * r(size) + (0.05 * k if name.endswith("b1") else 0.0)
                o += size
        self.theta = theta.to(DEV)
        n = self.n
        d = lambda t: t.to(device=DEV, dtype=torch.float64).contiguous()
        self.stats = dict(obs_mean=d(0.5 * r(K, 19)), obs_var=d(0.2 + r(K, 19).abs()), obs_count=d(50.0 + 100.0 * torch.rand(K, generator=g)),
                          ret_mean=d(r(K)), ret_var=d(0.3 + r(K).abs()), ret_count=d(20.0 + 100.0 * torch.rand(K, generator=g)), returns=d(2.0 * r(n)),
                          scratch=torch.zeros(K * L.POLICY_SCRATCH, dtype=torch.float64, device=DEV))
        obs = 1.5 * r(n, 19)
        obs[::3, 4] = 40.0                                             # some words beyond clip_obs
        self.obs = obs.to(DEV).contiguous()
        self.next_obs = (1.2 * r(n, 19) + 0.3).to(DEV).contiguous()
        self.prev_done = (torch.rand(n, generator=g) < 0.4).to(torch.uint8).to(DEV)
        self.done = (torch.rand(n, generator=g) < 0.3).to(torch.uint8).to(DEV)
        self.rew = (3.0 * r(n)).to(DEV).contiguous()
        self.low = torch.full((A,), -0.6, device=DEV)
        self.high = torch.linspace(0.3, 0.9, A, device=DEV).contiguous()
        self.ctr = torch.tensor([CTR_BASE], dtype=torch.int32, device=DEV)
        # the single-network side's packed weights come from the single-network pack: K launches of usim_policy_pack
        self.packed_single = torch.zeros(K, L.POLICY_PACKED, dtype=torch.float32, device=DEV)
        self.pack_single(self.theta, self.packed_single)
        self.packed_multi = torch.zeros(K, L.POLICY_PACKED, dtype=torch.float32, device=DEV)
        assert self.lib.usim_policy_pack_multi(self.theta.data_ptr(), self.stride, K, A, self.packed_multi.data_ptr(), _stream()) == 0

    # ---- the single-network calls on member k's slices ----
    def net(self, theta, k, packed):
        base, ptrs = theta.data_ptr() + 4 * k * self.stride, []
        for size in self.sizes:
            ptrs.append(base)
            base += 4 * size
        return self.usim._lib.UsimPolicyNet(*ptrs, None if packed is None else packed.data_ptr() + 4 * k * packed.shape[1])

    def pack_single(self, theta, packed):
        for k in range(self.K):
            net = self.net(theta, k, None)
            assert self.lib.usim_policy_pack(C.byref(net), packed.data_ptr() + 4 * k * packed.shape[1], _stream()) == 0

    def norm_stats(self, st, k=None):
        """usim_norm_stats of the K-major tensors `st`; with k, of member k's part of them"""
        G, S = self.G, self.usim._lib.POLICY_SCRATCH
        off = dict(obs_mean=19, obs_var=19, obs_count=1, ret_mean=1, ret_var=1, ret_count=1, returns=G, scratch=S)
        return self.usim._lib.UsimNormStats(*[st[name].data_ptr() + (0 if k is None else 8 * k * off[name]) for name in STAT_NAMES], 10.0, 5.0, 0.99, 1e-8)

    def outs(self):
        return {name: torch.full(((self.n + GUARD) * w,), SENTINEL, dtype=torch.float32, device=DEV)
                for name, w in zip(OUT_NAMES, (self.A, 19, self.A, 1, 1, 1))}

    def policy_out(self, o, k=None):
        G, w = self.G, dict(zip(OUT_NAMES, (self.A, 19, self.A, 1, 1, 1)))
        return self.usim._lib.UsimPolicyOut(*[o[name].data_ptr() + (0 if k is None else 4 * k * G * w[name]) for name in OUT_NAMES])

    def step(self, multi, training, deterministic, with_prev, with_base, theta=None, stats=None, obs=None, packed=None):
        """-> every output buffer (guards included) and every statistics tensor after the call, as int32 words"""
        K, G, A, lib = self.K, self.G, self.A, self.lib
        theta = self.theta if theta is None else theta
        obs = self.obs if obs is None else obs
        st = {k: v.clone() for k, v in (self.stats if stats is None else stats).items()}
        o = self.outs()
        base = self.ctr.data_ptr() if with_base else None
        if multi:
            packed = self.packed_multi if packed is None else packed
            S, out = self.norm_stats(st), self.policy_out(o)
            rc = lib.usim_policy_step_multi(theta.data_ptr(), self.stride, packed.data_ptr(), C.byref(S), obs.data_ptr(), self.prev_done.data_ptr() if with_prev else None,
                                            K, G, A, self.low.data_ptr(), self.high.data_ptr(), SEED, COUNTER, base, ENV_OFFSET, training, deterministic, C.byref(out), _stream())
            assert rc == 0
        else:
            packed = self.packed_single if packed is None else packed
            for k in range(K):
                net, S, out = self.net(theta, k, packed), self.norm_stats(st, k), self.policy_out(o, k)
                rc = lib.usim_policy_step(C.byref(net), C.byref(S), obs.data_ptr() + 4 * 19 * k * G, self.prev_done.data_ptr() + k * G if with_prev else None, G, A,
                                          self.low.data_ptr(), self.high.data_ptr(), SEED, COUNTER, base, ENV_OFFSET + k * G, training, deterministic, C.byref(out), _stream())
                assert rc == 0
        torch.cuda.synchronize()
        return {**{f"out.{k}": _bits(v) for k, v in o.items()}, **{f"stats.{k}": _bits(v) for k, v in st.items()}}

    def reward(self, multi, training, norm_reward, with_obs, stats=None, rew=None, next_obs=None):
        K, G, lib = self.K, self.G, self.lib
        rew = self.rew if rew is None else rew
        next_obs = self.next_obs if next_obs is None else next_obs
        st = {k: v.clone() for k, v in (self.stats if stats is None else stats).items()}
        nrew = torch.full((self.n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        raw = torch.arange(1, K + 1, dtype=torch.float64, device=DEV) * 0.37
        if multi:
            S = self.norm_stats(st)
            assert lib.usim_policy_reward_multi(C.byref(S), rew.data_ptr(), self.done.data_ptr(), K, G, training, norm_reward, nrew.data_ptr(), raw.data_ptr(),
                                                next_obs.data_ptr() if with_obs else None, _stream()) == 0
        else:
            for k in range(K):
                S = self.norm_stats(st, k)
                assert lib.usim_policy_reward(C.byref(S), rew.data_ptr() + 4 * k * G, self.done.data_ptr() + k * G, G, training, norm_reward, nrew.data_ptr() + 4 * k * G,
                                              raw.data_ptr() + 8 * k, next_obs.data_ptr() + 4 * 19 * k * G if with_obs else None, _stream()) == 0
        torch.cuda.synchronize()
        return {"nrew": _bits(nrew), "raw_sum": _bits(raw), **{f"stats.{k}": _bits(v) for k, v in st.items()}}


_CASES = {}


@pytest.fixture
def case(usim, request):
    key = request.param
    if key not in _CASES:
        _CASES[key] = Case(usim, *key)
    return _CASES[key]


def _all_cases():
    return [pytest.param((K, G, A), id=f"K{K}-G{G}-A{A}") for K, G in SHAPES for A in ADIMS]


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs in {int((a[k] != b[k]).sum())} of {a[k].numel()} words"


def _written(res, case):
    """the call wrote something: the outputs are no longer the sentinel (a comparison of two untouched buffers would pass too)"""
    v = res["out.value"].view(torch.float32)[:case.n]
    assert torch.isfinite(v).all() and (v != SENTINEL).all()


@pytest.mark.parametrize("case", _all_cases(), indirect=True)
def test_pack_multi_equals_the_member_packs(case):
    assert torch.equal(_bits(case.packed_multi), _bits(case.packed_single))
    assert case.packed_single.abs().sum().item() > 0 and (case.K == 1 or not torch.equal(case.packed_single[0], case.packed_single[-1]))


@pytest.mark.parametrize("case", _all_cases(), indirect=True)
def test_step_multi_equals_the_slice_calls(case):
    for training in (0, 1, 2):
        for deterministic in (0, 1):
            for with_prev in (False, True):
                with_base = not (training == 2 and deterministic and with_prev)          # (one combination without the device counter word)
                args = (training, deterministic, with_prev, with_base)
                multi, single = case.step(True, *args), case.step(False, *args)
                _written(multi, case)
                _same(multi, single, f"training {training} deterministic {deterministic} prev_done {with_prev} counter_base {with_base}")
    # the statistics moved when asked to, and only then; the noise depends on the counter word
    frozen, updated = case.step(True, 0, 0, True, True), case.step(True, 1, 0, True, True)
    assert torch.equal(frozen["stats.obs_mean"], _bits(case.stats["obs_mean"])) and not torch.equal(updated["stats.obs_mean"], frozen["stats.obs_mean"])
    assert not torch.equal(frozen["out.act"], case.step(True, 0, 0, True, False)["out.act"])


@pytest.mark.parametrize("case", _all_cases(), indirect=True)
def test_reward_multi_equals_the_slice_calls(case):
    for training in (0, 1):
        for norm_reward in (0, 1):
            for with_obs in (False, True):
                args = (training, norm_reward, with_obs)
                multi, single = case.reward(True, *args), case.reward(False, *args)
                assert (multi["nrew"].view(torch.float32)[:case.n] != SENTINEL).all()
                _same(multi, single, f"training {training} norm_reward {norm_reward} next_obs {with_obs}")
    trained = case.reward(True, 1, 1, True)
    assert not torch.equal(trained["stats.ret_var"], _bits(case.stats["ret_var"])) and not torch.equal(trained["stats.obs_mean"], _bits(case.stats["obs_mean"]))
    assert not torch.equal(trained["raw_sum"], _bits(torch.arange(1, case.K + 1, dtype=torch.float64, device=DEV) * 0.37))


def _member_words(res, case, k):
    """member k's words of a result: its rows of every per-environment buffer, its entries of the K-major statistics"""
    K, G, n = case.K, case.G, case.n
    out = {}
    for name, t in res.items():
        if name in ("out.act_env", "out.act", "out.nobs", "out.value", "out.logp", "out.start", "nrew"):
            w = t.numel() // (n + GUARD)
            out[name] = t[k * G * w:(k + 1) * G * w]
        else:
            w = t.numel() // K
            out[name] = t[k * w:(k + 1) * w]
    return out


@pytest.mark.parametrize("case", [pytest.param((3, 33, 6), id="K3-G33-A6"), pytest.param((2, 70, 7), id="K2-G70-A7")], indirect=True)
def test_a_nan_in_another_member_changes_nothing(case):
    K, G, bad = case.K, case.G, 1
    nan = float("nan")
    theta = case.theta.clone(); theta[bad, :case.P] = nan
    packed = torch.zeros_like(case.packed_multi)
    assert case.lib.usim_policy_pack_multi(theta.data_ptr(), case.stride, K, case.A, packed.data_ptr(), _stream()) == 0
    obs = case.obs.clone(); obs[bad * G:(bad + 1) * G] = nan
    next_obs = case.next_obs.clone(); next_obs[bad * G:(bad + 1) * G] = nan
    rew = case.rew.clone(); rew[bad * G:(bad + 1) * G] = nan
    stats = {k: v.clone() for k, v in case.stats.items()}
    for name in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count"):
        stats[name][bad] = nan
    stats["returns"][bad * G:(bad + 1) * G] = nan
    others = [k for k in range(K) if k != bad]
    for training in (0, 1):
        clean = case.step(True, training, 0, True, True)
        for what, kw in (("observations", dict(obs=obs)), ("weights", dict(theta=theta, packed=packed)), ("statistics", dict(stats=stats)),
                         ("all three", dict(obs=obs, theta=theta, packed=packed, stats=stats))):
            dirty = case.step(True, training, 0, True, True, **kw)
            assert torch.isnan(dirty["out.value"].view(torch.float32)[bad * G:(bad + 1) * G]).all(), what      # the NaN did reach its own member
            for k in others:
                _same(_member_words(dirty, case, k), _member_words(clean, case, k), f"training {training}, NaN in member {bad}'s {what}, member {k}")
    for with_obs in (False, True):
        clean = case.reward(True, 1, 1, with_obs)
        dirty = case.reward(True, 1, 1, with_obs, stats=stats, rew=rew, next_obs=next_obs)
        assert torch.isnan(dirty["nrew"].view(torch.float32)[bad * G:(bad + 1) * G]).all()
        for k in others:
            _same(_member_words(dirty, case, k), _member_words(clean, case, k), f"reward, next_obs {with_obs}, member {k}")
