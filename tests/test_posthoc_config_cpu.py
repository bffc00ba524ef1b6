"""CPU: `metrics=posthoc` composes, names the two post-hoc metric classes with the documented knobs, and leaves the default list as it
was; the two classes bind in the time view only and refuse what they cannot score before any engine call."""
import os
from functools import partial

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_posthoc_config_composes_and_names_the_two_classes():
    import fdiff.sampling.metrics as alias
    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.sampling.metrics import (DiscriminativeScore, MarginalWasserstein, MetricCollection, PredictiveScore,
                                                       SlicedWasserstein)
    assert alias.DiscriminativeScore is DiscriminativeScore and alias.PredictiveScore is PredictiveScore
    conf = os.path.join(ROOT, "cmd", "conf")
    default = compose(conf, "sample", []).metrics
    assert "holdout" not in default and [m["_target_"].rsplit(".", 1)[1] for m in default.metrics] == [
        "SlicedWasserstein", "MarginalWasserstein"]
    cfg = compose(conf, "sample", ["metrics=posthoc", "random_seed=7"]).metrics
    assert cfg.holdout is True
    make = instantiate({k: v for k, v in cfg.items() if k != "holdout"})
    assert isinstance(make, partial) and make.func is MetricCollection
    assert make.keywords["include_spectral_density"] is True and make.keywords["include_baselines"] is True
    assert [m.func for m in make.keywords["metrics"]] == [SlicedWasserstein, MarginalWasserstein, DiscriminativeScore, PredictiveScore]
    knobs = dict(steps=2000, batch_size=128, lr=0.001, d_model=32, num_layers=1, max_samples=10000, random_seed=7)
    assert make.keywords["metrics"][2].keywords == dict(knobs, test_fraction=0.2)
    assert make.keywords["metrics"][3].keywords == knobs
    assert [dict(m) for m in cfg.metrics[:2]] == [dict(m) for m in compose(conf, "sample", ["random_seed=7"]).metrics.metrics]


def test_classes_bind_in_the_time_view_and_take_a_holdout():
    import inspect

    from fourierdiffusion_amd.sampling.metrics import DiscriminativeScore, PredictiveScore
    for cls in (DiscriminativeScore, PredictiveScore):
        assert cls.views == ("time",)
        assert "holdout_samples" in inspect.signature(cls).parameters


@pytest.mark.parametrize("cls_name", ["DiscriminativeScore", "PredictiveScore"])
def test_classes_refuse_bad_arguments_before_any_engine_call(cls_name):
    import fourierdiffusion_amd.sampling.metrics as M
    cls = getattr(M, cls_name)
    x = np.zeros((8, 24, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="lost its time axis"):
        cls(x.reshape(8, 48))
    with pytest.raises(ValueError, match="at least two original"):
        cls(x[:1])
    with pytest.raises(ValueError, match="same number of features"):
        cls(x, holdout_samples=x[:, :12])
    with pytest.raises(ValueError, match="<= 100"):
        cls(x, d_model=128)
