"""Two-stage training, host side (no GPU): the trainable-range function on every configuration of tests/engine_cases.py, the
muting schedule's draw order, the float64 stage-two reference (tests/stage_ref.py), the numpy restatement of the muted gather
(tests/mute_ref.py) against feed_ref's, and the new entry point in the header, the binding and the built library."""
import os
import re

import numpy as np
import pytest
import torch

import engine_ref as R
import feed_ref as F
import gen_util as G
import mute_ref as M
import stage_ref as S
from engine_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 2e-3


def engine_shapes(case):
    from m2_mixer_amd import engine as E
    if case.engine == "mimic":
        return E.mimic_param_shapes(case.cfg)
    return E.two_tower_param_shapes(case.cfg, S.MODS[case.engine])


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_trainable_ranges_tile_the_flat_buffer_with_the_frozen_keys(case):
    from m2_mixer_amd import engine as E
    shapes = engine_shapes(case)
    assert list(shapes) == list(R.case_shapes(case))
    prefixes = E.frozen_key_prefixes(S.MODS[case.engine])
    assert set(prefixes) == set(S.frozen_prefixes(case))
    got = E.trainable_flat_ranges(shapes, prefixes)
    n_params = sum(int(torch.Size(s).numel()) for s in shapes.values())
    assert all(lo < hi for lo, hi in got)
    assert all(a[1] < b[0] for a, b in zip(got, got[1:])), "sorted, disjoint and merged (no two ranges touch)"
    frozen_keys = {k for k in shapes if S.is_frozen(case, k)}
    trainable_keys = set(shapes) - frozen_keys
    assert any(k.startswith("fusion_mixer.") for k in trainable_keys) and "classifier_fusion.classifer.weight" in trainable_keys
    a, b = S.MODS[case.engine]
    assert {f"classifier_{a}.weight", f"classifier_{a}.bias", f"classifier_{b}.weight", f"classifier_{b}.bias"} <= frozen_keys
    cover = np.zeros(n_params, dtype=np.int8)
    for lo, hi in got:
        cover[lo:hi] += 1
    for lo, hi in S.flat_ranges(shapes, frozen_keys):
        assert not cover[lo:hi].any(), "a frozen key inside a trainable range"
        cover[lo:hi] += 1
    assert (cover == 1).all(), "trainable and frozen ranges tile [0, n_params)"
    for lo, hi in S.flat_ranges(shapes, trainable_keys):
        assert any(a <= lo and hi <= b for a, b in got)
    # the two-tower layouts: everything from the fusion function to the fusion mixer, then the fusion head alone
    assert len(got) == 2


def test_trainable_ranges_by_hand():
    from m2_mixer_amd.engine import trainable_flat_ranges
    shapes = {"a_mixer.w": (2, 3), "fusion_function.g": (4,), "fusion_mixer.w": (5,), "classifier_a.weight": (2,), "classifier_fusion.classifer.bias": (3,)}
    assert trainable_flat_ranges(shapes, ("a_mixer.", "classifier_a.")) == [(6, 15), (17, 20)]
    assert trainable_flat_ranges(shapes, ()) == [(0, 20)]
    assert trainable_flat_ranges(shapes, ("a_mixer.", "fusion_", "classifier_")) == []


def test_muting_codes_consume_the_generator_as_shared_step_does():
    from m2_mixer_amd.models import muting_codes
    probs = {"image": 0.3, "audio": 0.2, "multimodal": 0.5}
    names = ["image", "audio", "multimodal"]
    np.random.seed(1234)
    got = muting_codes(40, probs, ("image", "audio"))
    after = np.random.random()
    np.random.seed(1234)
    want = [np.random.choice(names, p=[probs[n] for n in names]) for _ in range(40)]
    assert after == np.random.random(), "one draw per step, nothing else"
    assert got.dtype == np.int32 and got.tolist() == [{"image": 1, "audio": 2, "multimodal": 0}[str(w)] for w in want]
    assert set(got.tolist()) == {0, 1, 2}
    own = np.random.RandomState(7)
    twin = np.random.RandomState(7)
    assert muting_codes(5, probs, ("image", "audio"), rng=own).tolist() == \
        [{"image": 1, "audio": 2, "multimodal": 0}[str(twin.choice(names, p=[0.3, 0.2, 0.5]))] for _ in range(5)]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_frozen_step_keeps_frozen_keys_and_moves_the_rest(case):
    params = G.make_params(R.case_shapes(case), 31)
    ref = R.Step(case, params, LR)
    ref.step(R.case_batch(case, 101))
    two = S.FrozenStep(ref)
    before_p = {k: v.clone() for k, v in two.p.items()}
    before_m = {k: v.clone() for k, v in two.m.items()}
    before_v = {k: v.clone() for k, v in two.v.items()}
    out = two.step(R.case_batch(case, 102))
    assert two.t == 2 and float(out["losses"][3]) == float(out["losses"][2])
    for k in params:
        if S.is_frozen(case, k):
            assert torch.equal(two.p[k], before_p[k]) and torch.equal(two.m[k], before_m[k]) and torch.equal(two.v[k], before_v[k]), k
            assert k not in out["grads"]
        elif not k.endswith(R.NOISE_KEYS):
            assert not torch.equal(two.p[k], before_p[k]), f"{k} did not move"
    # stage one would have moved a frozen key on the same batch
    one = R.Step(case, params, LR)
    one.p, one.m, one.v = ({k: v.clone() for k, v in d.items()} for d in (before_p, before_m, before_v))
    one.t = 1
    one.step(R.case_batch(case, 102))
    assert any(not torch.equal(one.p[k], before_p[k]) for k in params if S.is_frozen(case, k))


def test_muted_gather_ref_agrees_with_the_plain_gather_when_nothing_is_muted():
    rng = np.random.default_rng(4)
    n, B = 11, 4
    a = rng.standard_normal((n, 5)).astype(np.float32)
    b = rng.integers(0, 256, size=(n, 12), dtype=np.uint8)
    y = rng.integers(0, 9, size=(n,), dtype=np.int64)
    perm = rng.permutation(n).astype(np.int32)
    state = np.array([0, 0, n, 0], dtype=np.uint32)
    mstate = np.array([0, 0], dtype=np.uint32)
    codes = np.zeros(3, dtype=np.int32)
    for k in range(4):                                   # the fourth gather wraps AND runs past the schedule
        want, after = F.gather((a, b, y), perm, state, B)
        got, state2, mstate = M.gather_muted((a, b, y), perm, state, B, codes, mstate)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and state2.tolist() == after.tolist()
        state = after
    assert mstate.tolist() == [4, 1] and state.tolist() == [16, 0, n, 1 + 5]      # 12 - 11, then 16 - 11
    # by hand: code 2 zeroes source 1 and nothing else
    got, _, ms = M.gather_muted((a, b, y), None, np.array([0, 0, n, 0], dtype=np.uint32), B, np.array([2]), np.array([0, 0], dtype=np.uint32))
    assert not got[1].any() and np.array_equal(got[0], F.raw(a[:4])) and np.array_equal(got[2], F.raw(y[:4])) and ms.tolist() == [1, 0]


def test_header_binding_and_library_carry_the_muted_gather():
    from m2_mixer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "m2mixer.h")).read()
    name = "m2m_feed_gather_muted"
    assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/m2mixer.h"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 9
    assert hasattr(_lib.lib(), name), f"{name} is not exported by the built library"
    assert int(re.search(r"#define M2M_FEED_MUTE_STATE_WORDS (\d+)", hdr).group(1)) == _lib.FEED_MUTE_STATE_WORDS == 2
    assert len(_lib.SIGNATURES["m2m_feed_gather"][1]) == 6                 # the plain gather keeps its signature
    assert _lib.lib().m2m_abi_version() == 18 == _lib.ABI_VERSION          # an addition within ABI 18
    assert int(re.search(r"#define M2M_ABI_VERSION (\d+)", hdr).group(1)) == 18


def test_muted_gather_refuses_bad_arguments_before_any_launch():
    """-1 with a message; the addresses below are only ever compared (validation comes before any launch)."""
    from m2_mixer_amd import _lib as L
    lib = L.lib()
    fake = 0x1000

    def src(**kw):
        d = (L.FeedSrc * 1)()
        d[0].src, d[0].dst, d[0].row_bytes = fake, fake, 16
        for k, v in kw.items():
            setattr(d[0], k, v)
        return d

    cases = [("NULL mute_state", lambda: lib.m2m_feed_gather_muted(src(), 1, 0, 4, fake, fake, 3, 0, 0), "mute_state"),
             ("NULL codes with ncodes > 0", lambda: lib.m2m_feed_gather_muted(src(), 1, 0, 4, fake, 0, 3, fake, 0), "needs codes"),
             ("ncodes < 0", lambda: lib.m2m_feed_gather_muted(src(), 1, 0, 4, fake, fake, -1, fake, 0), "ncodes"),
             ("NULL srcs", lambda: lib.m2m_feed_gather_muted(None, 1, 0, 4, fake, fake, 3, fake, 0), "srcs and state"),
             ("NULL state", lambda: lib.m2m_feed_gather_muted(src(), 1, 0, 4, 0, fake, 3, fake, 0), "srcs and state"),
             ("nsrc 5", lambda: lib.m2m_feed_gather_muted(src(), 5, 0, 4, fake, fake, 3, fake, 0), "nsrc"),
             ("B 0", lambda: lib.m2m_feed_gather_muted(src(), 1, 0, 0, fake, fake, 3, fake, 0), "B >= 1"),
             ("row_bytes 6", lambda: lib.m2m_feed_gather_muted(src(row_bytes=6), 1, 0, 4, fake, fake, 3, fake, 0), "row_bytes"),
             ("NULL dst", lambda: lib.m2m_feed_gather_muted(src(dst=0), 1, 0, 4, fake, fake, 3, fake, 0), "src and dst")]
    for what, call, msg in cases:
        assert call() == -1, what
        assert re.search(msg, lib.m2m_last_error().decode("utf-8", "replace")), what


def test_bind_engine_two_stage_is_a_keyword_with_default_off():
    import inspect
    from m2_mixer_amd.models import _MultiLossModule
    sig = inspect.signature(_MultiLossModule.bind_engine)
    assert sig.parameters["two_stage"].default is False
