"""The host side of the region term (gan_segmentation_amd/loss_ops.py): check_region, LossSpec(region=...), the
TRAIN_LOSS key with a region, and the defaults of region_loss."""
import inspect

import pytest

from gan_segmentation_amd import loss_ops
from gan_segmentation_amd.loss_ops import LossSpec

FULL = {"weight": 1.0, "alpha": 0.3, "beta": 0.7, "smooth": 0.0, "classes": "all"}


def test_check_region_defaults_and_accepted_values():
    assert loss_ops.check_region(None) is None
    assert loss_ops.check_region({"weight": 2}) == {"weight": 2.0, "alpha": 0.5, "beta": 0.5, "smooth": 1.0, "classes": "present"}
    assert loss_ops.check_region(dict(FULL)) == FULL
    got = loss_ops.check_region({"weight": 0, "alpha": 1, "beta": 1})
    assert got["weight"] == 0.0 and got["alpha"] == 1.0 and isinstance(got["alpha"], float) and got["smooth"] == 1.0
    assert loss_ops.check_region({"weight": 1, "alpha": 0, "beta": 1})["alpha"] == 0.0        # one of the two may be 0
    assert loss_ops.REGION_KEYS == ("weight", "alpha", "beta", "smooth", "classes")
    assert loss_ops.SPEC_KEYS == ("gamma", "normalise", "class_weights", "boundary", "region")


@pytest.mark.parametrize("v,key", [
    (3, "mapping"), ([("weight", 1)], "mapping"), ("dice", "mapping"),
    ({}, "weight"), ({"alpha": 0.5}, "weight"), ({"weight": -0.5}, "weight"), ({"weight": "1"}, "weight"), ({"weight": True}, "weight"),
    ({"weight": float("nan")}, "weight"), ({"weight": None}, "weight"),
    ({"weight": 1, "alpha": -0.1}, "alpha"), ({"weight": 1, "alpha": float("inf")}, "alpha"), ({"weight": 1, "alpha": "0.5"}, "alpha"),
    ({"weight": 1, "beta": -1}, "beta"), ({"weight": 1, "beta": None}, "beta"),
    ({"weight": 1, "alpha": 0, "beta": 0}, "alpha + beta"),
    ({"weight": 1, "smooth": -1e-6}, "smooth"), ({"weight": 1, "smooth": float("nan")}, "smooth"),
    ({"weight": 1, "classes": "some"}, "classes"), ({"weight": 1, "classes": 1}, "classes"), ({"weight": 1, "classes": None}, "classes"),
    ({"weight": 1, "gamma": 2}, "gamma"), ({"weight": 1, "smoothing": 1, "eps": 0}, "smoothing"),
])
def test_check_region_rejects_and_names_the_key(v, key):
    with pytest.raises(ValueError) as e:
        loss_ops.check_region(v)
    assert key in str(e.value) and str(e.value).startswith("region")
    with pytest.raises(ValueError) as e:
        LossSpec(region=v)
    assert key in str(e.value) and str(e.value).startswith("LossSpec: region")


def test_loss_spec_carries_the_region():
    assert LossSpec().region is None
    assert LossSpec().as_dict() == {"gamma": 0.0, "normalise": "mean", "class_weights": None, "boundary": None, "region": None}
    s = LossSpec(gamma=2, normalise="focal", class_weights="median", boundary={"weight": 4, "sigma": 2.0, "radius": 5}, region=dict(FULL))
    assert s.region == FULL and s.as_dict()["region"] == FULL and s.as_dict()["region"] is not s.region
    assert LossSpec.from_mapping(s.as_dict()).as_dict() == s.as_dict()
    assert LossSpec.from_mapping({"region": {"weight": 1}}).region["classes"] == "present"
    t = s.with_class_weights([1.0, 3.0])
    assert t.region == FULL and t.class_weights == (1.0, 3.0) and t.boundary == s.boundary and s.needs_masks and not t.needs_masks
    assert "region={'weight': 1.0" in repr(s) and "region=None" in repr(LossSpec())
    assert loss_ops.check_spec({"region": {"weight": 0.5}}).region["weight"] == 0.5
    with pytest.raises(ValueError) as e:
        LossSpec.from_mapping({"regions": {"weight": 1}})
    assert "regions" in str(e.value) and "region" in str(e.value).split("known:")[1]


def test_train_loss_key_with_a_region(tmp_path):
    from gan_segmentation_amd import main as cli
    spec = cli.check_train_loss({"region": {"weight": 1.0, "alpha": 0.3, "beta": 0.7}})
    assert isinstance(spec, LossSpec) and spec.gamma == 0.0
    assert spec.region == {"weight": 1.0, "alpha": 0.3, "beta": 0.7, "smooth": 1.0, "classes": "present"}
    for bad, word in (({"region": {"weight": -1}}, "weight"), ({"region": {"alpha": 0.3}}, "weight"), ({"region": 1.0}, "mapping"),
                      ({"region": {"weight": 1, "alpha": 0, "beta": 0}}, "alpha"), ({"region": {"weight": 1, "mode": "all"}}, "mode")):
        with pytest.raises(ValueError) as e:
            cli.check_train_loss(bad)
        assert "TRAIN_LOSS: region" in str(e.value) and word in str(e.value), (bad, str(e.value))
    # a bad region ends `train` before anything touches BASE_DIR or a device
    cfg = {"BASE_DIR": str(tmp_path / "nowhere"), "GAN": "ffhq", "GAN_GPU_IDS": [0], "TRAIN_LOSS": {"region": {"weight": 1, "smooth": -1}}}
    with pytest.raises(ValueError) as e:
        cli.train(cfg)
    assert "TRAIN_LOSS: region" in str(e.value) and "smooth" in str(e.value)
    assert "region" in cli.__doc__


def test_fit_checks_a_region_before_reading_a_sample(tmp_path):
    from gan_segmentation_amd.seg_solver import SegSolver
    solver = object.__new__(SegSolver)
    solver.cfg = {"num_classes": 2}
    solver.path_to_data = str(tmp_path / "missing")
    with pytest.raises(ValueError) as e:
        solver.fit(loss={"region": {"weight": 1, "classes": "every"}})
    assert str(e.value).startswith("loss: region") and "classes" in str(e.value)
    with pytest.raises(FileNotFoundError):
        solver.fit(loss={"region": {"weight": 1}})


def test_region_loss_defaults_and_host_tensors():
    import torch
    p = inspect.signature(loss_ops.region_loss).parameters
    assert [p[k].default for k in ("alpha", "beta", "smooth", "classes", "class_weights", "grad", "grad_scale", "into", "workspace")] \
        == [0.5, 0.5, 1.0, "present", None, True, 1.0, None, None]
    with pytest.raises(ValueError):
        loss_ops.region_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int8))
