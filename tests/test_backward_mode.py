"""CPU suite of the backward modes' host layer (nerf-pytorch_amd/backward_mode.py and its callers): the vocabulary, the "auto"
policy with its probe, the fold of the statistics words, and what FlexibleNeRFModel keeps of a choice across plan changes and
copies.  Plans and models are host objects: no GPU is needed."""
import copy
import io
import os
import pickle
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import nerf_pytorch_amd as N  # noqa: E402
from nerf_pytorch_amd import _lib as L  # noqa: E402
from nerf_pytorch_amd import backward_mode as BM  # noqa: E402

FERN = dict(num_layers=4, hidden_size=64, skip_connect_every=3, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)   # config/fern.yml's nets


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "nerf-pytorch_amd", "csrc"), "lib", "-j8"], check=True)
    return L.get_lib()


def test_parse_accepts_exactly_the_documented_spellings():
    assert BM.NAMES == ("dense", "compact", "recompute", "fused", "fused_compact", "fused_stash")
    for code, name in enumerate(BM.NAMES):
        assert BM.parse(name) == code and BM.parse(code) == code and type(BM.parse(code)) is int
    assert (BM.parse(True), BM.parse(False), BM.parse(1), BM.parse(0)) == (1, 0, 1, 0) and type(BM.parse(True)) is int
    for bad in ("gather", "Dense", "fused-stash", "auto", 6, -1, 2.0, None, b"dense", [1]):
        with pytest.raises(ValueError, match="fused_stash"):   # (the message names the accepted values)
            BM.parse(bad)
    assert sorted(BM.BUILDS_LIST) == [1, 2, 4] and sorted(BM.FUSED_MODES) == [3, 4, 5] and BM.PROBE_EVERY == 50


def test_policy_with_probe_substitutes_the_list_building_mode():
    fracs = (None, 0.0, 0.04, 0.05, 0.10, 0.15, 0.29, 0.30, 0.5, 0.71, 0.72, 0.99)
    seen = set()
    for f16 in (False, True):
        for fused in (0, 3, 5):
            for frac in fracs:
                plain = BM.choose(frac, f16, fused)
                assert plain == N.TrainEngine._mode_for(frac, f16, fused) == BM.choose(frac, f16, fused, probe=False)
                want = {0: 1, 3: 4, 5: 4}.get(plain, plain)
                assert BM.choose(frac, f16, fused, probe=True) == want, (frac, f16, fused, plain)
                seen.add(plain)
    assert seen == {0, 1, 2, 3, 4, 5}


def test_fold_ignores_pairs_no_backward_wrote():
    assert BM.fold(None, 10, 40) == 0.75 and BM.fold(0.2, 40, 40) == 0.0 and BM.fold(0.2, 0, 40) == 1.0
    for kept, total in ((0, 0), (41, 40), (-1, 40), (5, -3)):
        assert BM.fold(0.25, kept, total) == 0.25 and BM.fold(None, kept, total) is None, (kept, total)
    r = BM.StatsReader(("coarse", "fine"))
    assert r.frac == {"coarse": None, "fine": None}
    r.poll()   # (nothing in flight: nothing to fold)
    assert r.frac == {"coarse": None, "fine": None}


def test_set_backward_compaction_sets_the_named_mode(lib):
    wide, fern = N.FlexibleNeRFModel(), N.FlexibleNeRFModel(**FERN)
    assert wide.backward_compaction == 0 and fern.backward_compaction == fern.fused_backward_available() == 5
    for m, values in ((wide, ("dense", 0, 2, "recompute", True, "compact", False)), (fern, ("dense", 0, 2, "recompute", 3, 4, 5) + BM.NAMES)):
        for x in values:
            assert m.set_backward_compaction(x) is m
            assert m.backward_compaction == lib.plan_bwd_compaction(m._plan) == BM.parse(x) == m._backward_choice, x
    for bad in ("gather", "Dense", 6, 2.0, None):
        with pytest.raises(ValueError):
            fern.set_backward_compaction(bad)
    assert fern.backward_compaction == lib.plan_bwd_compaction(fern._plan) == 5 and fern._backward_choice == 5
    # a fused mode on a plan that has none is refused, and nothing has changed
    wide.set_backward_compaction("recompute")
    with pytest.raises(L.NerfHipError, match="fused backward"):
        wide.set_backward_compaction("fused")
    assert wide._backward_choice == 2 and wide.backward_compaction == lib.plan_bwd_compaction(wide._plan) == 2


def test_the_choice_is_resolved_again_when_the_plan_changes(lib):
    """A 4x64 model in "auto" followed by set_training_precision("f16x3_train") used to raise from the new plan (the fused backward
    exists for fp32 plans only) after the model had been taken apart; an explicit fused choice is now refused while it is intact."""
    torch.manual_seed(3)
    m = N.FlexibleNeRFModel(**FERN)
    before, keys = m.flat_params.clone(), list(m.state_dict().keys())
    m.set_backward_compaction("auto")
    assert m.backward_compaction == 5 and m._auto_frac is None
    assert m.set_training_precision("f16x3_train") is m
    assert m.training_precision == "f16x3_train" and m.backward_compaction == lib.plan_bwd_compaction(m._plan) == 0
    assert isinstance(m.flat_params, torch.Tensor) and torch.equal(m.flat_params, before) and list(m.state_dict().keys()) == keys
    m.set_training_precision("fp32")
    assert m._backward_choice == "auto" and m.backward_compaction == m.fused_backward_available() == lib.plan_bwd_compaction(m._plan) == 5
    m.set_backward_compaction("fused")
    with pytest.raises(L.NerfHipError, match="fused backward"):
        m.set_training_precision("f16x3_train")
    assert m.training_precision == "fp32" and m.backward_compaction == lib.plan_bwd_compaction(m._plan) == 3 and m._backward_choice == 3
    assert torch.equal(m.flat_params, before) and list(m.state_dict().keys()) == keys
    m.set_backward_compaction("recompute")   # (a mode every plan has travels to the new plan)
    m.set_training_precision("f16x3_train")
    assert m.backward_compaction == lib.plan_bwd_compaction(m._plan) == 2 and torch.equal(m.flat_params, before)


@pytest.mark.parametrize("choice,mode", [("auto", 5), ("fused_compact", 4), (False, 0)])
def test_copies_keep_the_choice_and_the_plans_mode(lib, choice, mode):
    m = N.FlexibleNeRFModel(**FERN).set_backward_compaction(choice)
    if choice == "auto":
        m._stats.frac["net"] = 0.25   # (what a backward has reported travels; a copy in flight would not)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m)), torch.load(buf, weights_only=False)):
        assert c._plan != m._plan and c._backward_choice == m._backward_choice
        assert c.backward_compaction == lib.plan_bwd_compaction(c._plan) == mode
        assert c._auto_frac == (0.25 if choice == "auto" else None)
        if choice == "auto":
            assert c._stats is not m._stats and c._stats._host is None and c._stats._event is None
        assert torch.equal(c.flat_params, m.flat_params)


def test_the_mode_vocabulary_lives_in_one_module():
    pkg = os.path.join(ROOT, "nerf-pytorch_amd")
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py") and fn != "backward_mode.py":
            src = open(os.path.join(pkg, fn)).read()
            for literal in ("(1, 2, 4)", "(3, 5)", "int(bool(on))"):
                assert literal not in src, (fn, literal)
    assert "from .engine import" not in open(os.path.join(pkg, "models.py")).read()
