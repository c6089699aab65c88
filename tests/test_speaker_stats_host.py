"""Host side of the speaker statistics (speechdrivestemplates_amd/speaker_stats.py): csv selection and chunking,
the npz round trip into get_speaker_stat, DATASET.SPEAKER_STAT_FILE, the loud failures that need no GPU, the re-registration regression
of PoseTransforms._stat, and a float64 restatement of the kernels' arithmetic against the reference's recorded statistics."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import synth_speaker_stats as S  # noqa: E402

from speechdrivestemplates_amd import speaker_stats as SS  # noqa: E402
from speechdrivestemplates_amd.config import get_cfg_defaults  # noqa: E402
from speechdrivestemplates_amd.core.datasets import gesture_dataset as gd  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "speaker_stats_reference.npz")
PART_ROOT = np.full(137, -1)
PART_ROOT[95:116], PART_ROOT[116:137], PART_ROOT[25:55], PART_ROOT[56:95] = 7, 4, 55, 55


def contract_stats(paths, num_chunks, F=64):
    """the arithmetic of csrc/speaker_stats.hip in numpy, lanes (chunk, frame, keypoint) vectorised, clips in order
    -> {mode: (mean137 (2, 137), std137 (2, 137))}"""
    stride = len(paths) // num_chunks
    clips = [[SS.read_clip_poses(paths[c * stride + j], F) for j in range(stride)] for c in range(num_chunks)]

    def q_of(P):  # P (C, F, 2, 137) in the file dtype -> root (C, F, 2, 1), parted q, global q
        root = P[..., 1:2]
        g = P - root
        g[..., 1] = P[..., 1]
        pr = PART_ROOT >= 0
        q = g.copy()
        q[..., pr] = g[..., pr] - (P[..., PART_ROOT[pr]] - root)
        return root, q, g

    def run(M):
        st = {m: [np.zeros((num_chunks, F, 137)), np.zeros((num_chunks, F, 2, 137))] for m in ('parted', 'global')}
        for j in range(stride):
            P = np.stack([clips[c][j] for c in range(num_chunks)])
            root, qp, qg = q_of(P)
            for m, q in (('parted', qp), ('global', qg)):
                keep = ~((np.abs(q[..., 0, :] + root[..., 0, :]) < 5) & (np.abs(q[..., 1, :] + root[..., 1, :]) < 5))
                n, a = st[m]
                w = n / (n + 1.0)
                om = 1.0 - w
                v = q.astype(np.float64)
                if M is not None:
                    v = (v - M[m]) * (v - M[m])
                new = a * w[..., None, :] + om[..., None, :] * v
                a[:] = np.where(keep[..., None, :], new, a)
                n[:] = np.where(keep, n + 1.0, n)
        return st

    def reduce(st, sqrt):
        out = {}
        for m, (n, a) in st.items():
            a = np.sqrt(a) if sqrt else a
            s = a[0].copy()
            for c in range(1, num_chunks):
                s = s + a[c]
            s = s / num_chunks
            t = s[0].copy()
            for f in range(1, F):
                t = t + s[f]
            out[m] = t / F
        return out

    mean = reduce(run(None), False)
    std = reduce(run(mean), True)
    return {m: (mean[m], std[m]) for m in mean}


@pytest.fixture(scope="module")
def speakers(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("speakers"))
    for sp in S.SPEAKERS:
        S.write_named(root, sp)
    return root


@pytest.mark.parametrize("case", sorted(S.CASES))
def test_contract_restatement_matches_reference_bits(speakers, case):
    """the kernels' operation order (file-dtype root deduction, float64 recurrences, sequential chunk then frame averages) gives
    the reference's recorded bits; the GPU tests hold the kernels to the same fixture"""
    z = np.load(FIXTURE)
    sp, C = S.CASES[case]
    plan = SS.plan_speaker_stats(speakers, sp, num_chunks=C)
    got = contract_stats(plan['paths'], C)
    for m in ('parted', 'global'):
        assert np.array_equal(got[m][0], z['%s/%s_mean137' % (case, m)]), (case, m, 'mean')
        assert np.array_equal(got[m][1], z['%s/%s_std137' % (case, m)]), (case, m, 'std')
    assert int(z[case + '/clips_used']) == plan['clips_used'] and int(z[case + '/clips_dropped']) == plan['clips_dropped']


def test_plan_selects_train_rows_in_csv_order_and_drops_the_remainder(tmp_path):
    root = str(tmp_path)
    S.write_stats_speaker(root, "sp", n_train=23, seed=5, features=False, audio_len=16)
    import pandas as pd
    df = pd.read_csv(os.path.join(root, "sp", "processed_137.csv"))
    train = [os.path.join(root, "sp", f) for f in df[df["dataset"] == "train"]["pose_fn"]]
    assert len(df) > len(train) == 23
    for C, stride, dropped in ((10, 2, 3), (3, 7, 2), (1, 23, 0), (23, 1, 0)):
        p = SS.plan_speaker_stats(root, "sp", num_chunks=C)
        assert p['paths'] == train and p['stride'] == stride and p['clips_dropped'] == dropped and p['clips_used'] == 23 - dropped
    # --csv selects another clip list in the same directory (4_1 itself reads clips.csv)
    df[df["dataset"] == "train"][:5].to_csv(os.path.join(root, "sp", "clips.csv"), index=False)
    p = SS.plan_speaker_stats(root, "sp", csv="clips.csv", num_chunks=2)
    assert p['paths'] == train[:5] and p['stride'] == 2 and p['clips_dropped'] == 1
    # an absolute pose_fn stays as it is (os.path.join)
    df.loc[0, "pose_fn"] = os.path.join(root, "sp", df.loc[0, "pose_fn"])
    df.to_csv(os.path.join(root, "sp", "abs.csv"), index=False)
    assert SS.plan_speaker_stats(root, "sp", csv="abs.csv", num_chunks=1)['paths'] == train


def test_too_few_clips_and_short_clips_raise(tmp_path):
    root = str(tmp_path)
    S.write_stats_speaker(root, "few", n_train=4, seed=6, features=False, audio_len=16)
    with pytest.raises(ValueError, match="4 training clips, fewer than num_chunks=10"):
        SS.compute_speaker_stats(root, "few", scale_factor=1.0)
    S.write_stats_speaker(root, "short", n_train=5, seed=7, features=False, short_row=0, audio_len=16)
    with pytest.raises(ValueError, match=r"clips/00000\.npz: 40 frames, fewer than the 64"):
        SS.compute_speaker_stats(root, "short", num_chunks=1, scale_factor=1.0)
    S.write_stats_speaker(root, "short3", n_train=5, seed=7, features=False, short_row=3, audio_len=16)
    with pytest.raises(ValueError, match=r"clips/00004\.npz: 40 frames"):
        SS.read_clip_poses(os.path.join(root, "short3", "clips", "00004.npz"), 64)
    with pytest.raises(ValueError, match="exactly one of scale_factor"):
        SS.compute_speaker_stats(root, "short", num_chunks=1)
    with pytest.raises(KeyError, match="no built-in"):
        SS.compute_speaker_stats(root, "short", num_chunks=1, scale_like="no_such_speaker")


def _stats(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return {'parted': {'mean': rng.standard_normal(242) * 20, 'std': rng.uniform(2, 30, 242), 'scale_factor': 0.9549},
            'global': {'mean': rng.standard_normal(242) * 60, 'std': rng.uniform(5, 80, 242), 'scale_factor': 1.25},
            'counts': np.arange(274, dtype=np.int64).reshape(2, 137), 'num_chunks': 10, 'num_frames': 64, 'clips_used': 20,
            'clips_dropped': 3, 'csv': '/data/sp/processed_137.csv'}


def test_save_load_round_trip_into_get_speaker_stat(tmp_path):
    st = _stats(1)
    path = SS.save_speaker_stats(str(tmp_path / "s.npz"), st)
    z = np.load(path)
    assert {'parted_mean', 'parted_std', 'parted_scale', 'global_mean', 'global_std', 'global_scale'} <= set(z.files)
    assert int(z['clips_dropped']) == 3 and int(z['num_chunks']) == 10 and str(z['source_csv']) == st['csv']
    gd.load_speaker_stats(path, "roundtrip_speaker")
    pt = gd.PoseTransforms()
    for mode, parted in (('parted', True), ('global', False)):
        got = pt.get_speaker_stat("roundtrip_speaker", 121, parted)
        assert np.array_equal(got['mean'], st[mode]['mean']) and np.array_equal(got['std'], st[mode]['std'])
        assert got['scale_factor'] == st[mode]['scale_factor']


def test_speaker_stat_file_makes_an_unknown_speaker_resolvable(tmp_path):
    root = str(tmp_path)
    S.write_stats_speaker(root, "custom_host_speaker", n_train=3, seed=8, features=False)
    path = SS.save_speaker_stats(str(tmp_path / "custom.npz"), _stats(2))
    cfg = get_cfg_defaults()
    cfg.merge_from_list(["DATASET.ROOT_DIR", root, "DATASET.SPEAKER", "custom_host_speaker"])
    ds = gd.GestureDataset(root, "custom_host_speaker", "train", cfg)
    with pytest.raises(KeyError, match="no parted statistics"):
        ds[0]
    cfg.merge_from_list(["DATASET.SPEAKER_STAT_FILE", path])
    gd.register_configured_speaker_stats(cfg)
    item = gd.GestureDataset(root, "custom_host_speaker", "train", cfg)[0]
    assert np.array_equal(item['speaker_stat']['mean'], _stats(2)['parted']['mean'])
    assert torch.isfinite(item['poses']).all()
    assert get_cfg_defaults().DATASET.SPEAKER_STAT_FILE is None


def test_rehome_does_not_let_an_old_table_overwrite_a_new_one():
    """register A, use A, register B, use B, use A, use B -> B (the old array's refresh wrote A's values into the tensor
    that B's entry shared)"""
    class T(gd.PoseTransforms):
        pass
    t = T()
    t.cfg = get_cfg_defaults().DATASET
    kp = torch.zeros(1, 2, 121)
    ones, tens = np.ones(242), np.full(242, 10.0)
    A = {'mean': np.zeros(242), 'std': ones.copy(), 'scale_factor': 1.0}
    B = {'mean': np.zeros(242), 'std': tens.copy(), 'scale_factor': 1.0}
    gd.register_speaker_stat("rehome_speaker", parted=A)
    assert float(t._stat(A['std'], kp)[0, 0, 0]) == 1.0
    gd.register_speaker_stat("rehome_speaker", parted=B)
    assert float(t._stat(B['std'], kp)[0, 0, 0]) == 10.0
    assert float(t._stat(A['std'], kp)[0, 0, 0]) == 1.0
    assert float(t._stat(B['std'], kp)[0, 0, 0]) == 10.0
    assert float(t._stat(gd.SPEAKERS_STAT_121_parted["rehome_speaker"]['std'], kp)[0, 0, 0]) == 10.0


def test_c_abi_checks_sizes_before_launching():
    """sdt_speaker_stats_*: the state size query and the argument checks (they return before touching the GPU)"""
    import ctypes
    from speechdrivestemplates_amd import _lib
    lib = _lib.load()
    assert lib.sdt_speaker_stats_state_bytes(10, 64) == 7 * 10 * 64 * 137 * 8
    assert lib.sdt_speaker_stats_state_bytes(0, 64) == 0 and lib.sdt_speaker_stats_state_bytes(3, 0) == 0
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its checks
    sb = lib.sdt_speaker_stats_state_bytes(3, 64)
    clip = 64 * 274
    ok = dict(pss=1, eb=8, elems=3 * 7 * clip, pitch=7 * clip, C=3, F=64, w=7, j0=0, rows=7, sb=sb)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sdt_speaker_stats_accumulate(a['pss'], a['eb'], p, a['elems'], a['pitch'], a['C'], a['F'], a['w'], a['j0'], a['rows'],
                                                None, p, a['sb'], None)
    for bad in (dict(elems=3 * 7 * clip - 1), dict(pitch=7 * clip - 1), dict(j0=1), dict(w=8), dict(sb=sb - 8), dict(eb=2), dict(pss=3),
                dict(pss=2), dict(F=4096), dict(C=0)):
        assert call(**bad) == -1, bad
        assert b"sdt_speaker_stats_accumulate" in lib.sdt_last_error()
    assert lib.sdt_speaker_stats_finalize(1, p, sb - 8, 3, 64, p, p, p, p, p, None) == -1
    assert lib.sdt_speaker_stats_finalize(1, p, sb, 3, 64, p, None, p, p, p, None) == -1
