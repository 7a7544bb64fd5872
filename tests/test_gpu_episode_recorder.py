"""usim_record_step (csrc/usim_metrics.hip): synthetic inputs through the C ABI against tests/metrics_ref.py RecorderRef, bit for bit -- tracked indices that are
out of range, a time word that is out of range, more episodes than slots --, then evaluation.EpisodeRecorder on the simulator against episode_log.EpisodeLogger:
the same CSV files, byte for byte."""
import ctypes as C
import filecmp

import numpy as np
import pytest
import torch

import metrics_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5AA5A5
GUARD = 64


@pytest.mark.parametrize("n,indices,episodes", [(20, [3, 25, 0, -1, 19], 2), (1, [0], 1), (70, list(range(69, -1, -1)), 3)])
def test_synthetic_sequences_bit_for_bit(usim, n, indices, episodes):
    L, lib = usim._lib, usim._lib.load()
    H, m = 7, len(indices)
    words = L.record_words(m, episodes, H)
    assert lib.usim_record_words(m, episodes, H) == words
    buf = torch.cat([torch.zeros(words, dtype=torch.int32), torch.full((GUARD,), SENTINEL, dtype=torch.int32)]).to(DEV)
    index = torch.tensor(indices, dtype=torch.int32, device=DEV)
    rec = ref.RecorderRef(n, indices, episodes, H)
    seq = ref.synthetic_episodes(n, H, 30, seed=n + episodes, p_done=0.2)
    seq[4][0][0, ref.TIME] = np.float32(9 / 7 * 100.0)                # t = 9: outside [0, 7), no row is copied
    seq[5][0][0, ref.TIME] = np.float32(-3 / 7 * 100.0)               # t = -3
    seq[6][0][0, ref.TIME] = np.float32("nan")
    seq[6][1][0] = 1                                                  # ... and the episode closes on it: no length
    keep = []
    for k, (log, done) in enumerate(seq):
        dl, dd = torch.from_numpy(log).to(DEV).contiguous(), torch.from_numpy(done).to(DEV)
        keep.append((dl, dd))
        io = L.UsimStepIO(None, None, None, dd.data_ptr(), None, None, None, None, None, None, dl.data_ptr())
        assert lib.usim_record_step(C.byref(io), n, H, index.data_ptr(), m, episodes, buf.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        rec.step(log, done)
        if k in (3, 6, 29):
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert (got[words:].view(np.uint32) == SENTINEL).all(), "words behind the block were written"
            np.testing.assert_array_equal(got[:words], rec.block())
    good = [r for r, e in enumerate(indices) if 0 <= e < n]
    assert (rec.filled[good] == episodes).all() and (np.delete(rec.filled, good) == 0).all()          # every slot was filled, and then nothing more was recorded
    filled, lengths, rows = usim.evaluation.EpisodeRecorder.episodes_from_block(buf[:words].cpu().numpy(), m, episodes, H)
    np.testing.assert_array_equal(filled, rec.filled)
    np.testing.assert_array_equal(lengths, rec.lengths)
    np.testing.assert_array_equal(rows.view(np.uint32), rec.rows.view(np.uint32))


def test_recorder_writes_the_loggers_files_on_the_simulator(usim, tmp_path):
    """16 environments, horizon 60, 200 random-action steps: environments 5 and 9 recorded on the device, environment 5 also followed by the host-side logger"""
    kw = usim.default_robosuite_kwargs(); kw["horizon"] = 60
    env = usim.UltrasoundVecEnv(16, device=DEV, seed=11, **kw)
    rec = env.attach_observer(usim.EpisodeRecorder(env, [5, 9], episodes=2))
    logger = usim.episode_log.EpisodeLogger(env, env_index=5, root=str(tmp_path / "logger"))
    assert env.observers == (rec,) and not rec.complete()
    with pytest.raises(ValueError):
        env.attach_observer(rec)                                      # twice
    with pytest.raises(ValueError):
        usim.EpisodeRecorder(env, [5, 5])
    with pytest.raises(ValueError):
        usim.EpisodeRecorder(env, [16])
    env.reset_tensor()
    ends = 0
    for k in range(200):
        _, _, done = env.step_tensor(env.random_actions_tensor(k))
        d5 = bool(done[5])
        logger.after_step(d5)
        ends += d5
    assert ends >= 3 and rec.complete()                               # an episode lasts at most 60 steps
    eps = rec.episodes()
    assert [(e["env"], e["index"]) for e in eps] == [(5, 0), (5, 1), (9, 0), (9, 1)]
    for e in eps:
        assert 1 <= e["length"] <= 60 and e["rows"].shape == (60, 53) and e["rows"].dtype == np.float32
        assert (e["rows"][e["length"]:] == 0).all() and e["rows"][e["length"] - 1].any()
    written = rec.write_csv(str(tmp_path / "recorder"))
    assert len(written) == 23 * 4
    for folder, stem, _, _ in usim.episode_log._CHANNELS:
        for idx in (1, 2):                                            # environment 5's first two episodes are the recorder's files 1 and 2
            a, b = tmp_path / "recorder" / folder / f"{stem}_{idx}.csv", tmp_path / "logger" / folder / f"{stem}_{idx}.csv"
            assert filecmp.cmp(a, b, shallow=False), (folder, stem, idx)
    assert env.detach_observer(rec) is rec and env.observers == ()
    rec.reset()
    assert not rec.complete() and rec.episodes() == []
    env.close()
