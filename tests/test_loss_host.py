"""The host side of the decoder losses (gan_segmentation_amd/loss_ops.py): the boundary weight table, the
validation of LossSpec, of the TRAIN_LOSS key and of fit(loss=...), and the class weights from masks against pair_stats.summarise."""
import inspect

import numpy as np
import pytest

from gan_segmentation_amd import loss_ops, pair_stats
from gan_segmentation_amd.loss_ops import LossSpec


# ---- the boundary table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,weight,sigma", [(1, 4.0, 1.0), (3, 2.5, 1.5), (8, 0.0, 2.0), (32, 10.0, 11.3), (32, 1.0, 0.1)])
def test_boundary_weight_table_is_the_float64_formula_rounded_once(radius, weight, sigma):
    t = loss_ops.boundary_weight_table(radius, weight, sigma)
    assert t.dtype == np.float32 and t.shape == (1026,) == (loss_ops.LOSS_TABLE,)
    for d in range(1026):
        inside = 1 <= d <= radius * radius
        want = np.float32(1.0 + weight * np.exp(-np.float64(d) / (2.0 * np.float64(sigma) ** 2))) if inside else np.float32(1.0)
        assert t[d] == want, (d, t[d], want)
    assert t[0] == 1.0 and t[1025] == 1.0 and (t[radius * radius + 1:] == 1.0).all()
    assert (t >= 1.0).all() and (np.diff(t[1:radius * radius + 1]) <= 0).all()
    if weight > 0 and sigma > 0.5:
        assert t[1] > 1.0


def test_boundary_weight_table_covers_the_largest_radius():
    assert loss_ops.MAX_RADIUS ** 2 == loss_ops.LOSS_TABLE - 2
    from gan_segmentation_amd import mask_ops
    assert loss_ops.MAX_RADIUS == mask_ops.BOUNDARY_MAX_RADIUS and mask_ops.BOUNDARY_FAR > loss_ops.LOSS_TABLE


@pytest.mark.parametrize("kw", [dict(radius=0), dict(radius=33), dict(radius=2.0), dict(radius=True), dict(weight=-0.1),
                                dict(weight=float("nan")), dict(weight="1"), dict(sigma=0.0), dict(sigma=-1.0),
                                dict(sigma=float("inf")), dict(sigma=None)])
def test_boundary_weight_table_rejects(kw):
    with pytest.raises(ValueError):
        loss_ops.boundary_weight_table(**dict(dict(radius=3, weight=1.0, sigma=1.0), **kw))


# ---- LossSpec ---------------------------------------------------------------------------------------------------------------
def test_loss_spec_defaults_and_accepted_values():
    s = LossSpec()
    assert (s.gamma, s.normalise, s.class_weights, s.boundary) == (0.0, "mean", None, None) and s.table() is None and not s.needs_masks
    s = LossSpec(gamma=2, normalise="focal", class_weights=[0.5, 2], boundary={"weight": 4, "sigma": 2.0, "radius": 5})
    assert s.gamma == 2.0 and isinstance(s.gamma, float) and s.class_weights == (0.5, 2.0)
    assert s.boundary == {"weight": 4.0, "sigma": 2.0, "radius": 5}
    assert np.array_equal(s.table(), loss_ops.boundary_weight_table(5, 4.0, 2.0))
    for g in (0, 0.0, 1, 1.0, 3.5, 8, np.float32(2.0)):
        assert LossSpec(gamma=g).gamma == float(g)
    for nm in ("mean", "valid", "focal"):
        assert LossSpec(normalise=nm).normalise == nm
    for scheme in ("median", "inverse"):
        s = LossSpec(class_weights=scheme)
        assert s.needs_masks and s.class_weights == scheme
        t = s.with_class_weights([1.0, 3.0])
        assert not t.needs_masks and t.class_weights == (1.0, 3.0) and s.class_weights == scheme
    assert LossSpec(class_weights=np.array([1.0, 0.0, 2.0])).class_weights == (1.0, 0.0, 2.0)
    assert len(LossSpec(class_weights=[1.0] * 64).class_weights) == 64
    assert LossSpec.from_mapping(LossSpec(gamma=2, class_weights=[1, 2]).as_dict()).as_dict() == LossSpec(gamma=2, class_weights=[1, 2]).as_dict()


@pytest.mark.parametrize("kw,key", [
    (dict(gamma=0.5), "gamma"), (dict(gamma=-1), "gamma"), (dict(gamma=8.01), "gamma"), (dict(gamma="2"), "gamma"),
    (dict(gamma=True), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(gamma=None), "gamma"),
    (dict(normalise="sum"), "normalise"), (dict(normalise=1), "normalise"), (dict(normalise=None), "normalise"),
    (dict(class_weights="mean"), "class_weights"), (dict(class_weights=[1.0]), "class_weights"),
    (dict(class_weights=[1.0] * 65), "class_weights"), (dict(class_weights=[1.0, -1.0]), "class_weights"),
    (dict(class_weights=[1.0, float("inf")]), "class_weights"), (dict(class_weights=[1.0, "2"]), "class_weights"),
    (dict(class_weights=[1.0, None]), "class_weights"), (dict(class_weights=3.0), "class_weights"),
    (dict(boundary=3), "boundary"), (dict(boundary={"weight": 1.0, "sigma": 1.0}), "radius"),
    (dict(boundary={"weight": 1.0, "sigma": 1.0, "radius": 2, "shape": "gauss"}), "shape"),
    (dict(boundary={"weight": -1.0, "sigma": 1.0, "radius": 2}), "weight"),
    (dict(boundary={"weight": 1.0, "sigma": 0, "radius": 2}), "sigma"),
    (dict(boundary={"weight": 1.0, "sigma": 1.0, "radius": 0}), "radius"),
    (dict(boundary={"weight": 1.0, "sigma": 1.0, "radius": 33}), "radius"),
    (dict(boundary={"weight": 1.0, "sigma": 1.0, "radius": 2.5}), "radius"),
])
def test_loss_spec_rejects_and_names_the_key(kw, key):
    with pytest.raises(ValueError) as e:
        LossSpec(**kw)
    assert key in str(e.value) and str(e.value).startswith("LossSpec")


# ---- TRAIN_LOSS and fit(loss=...) ---------------------------------------------------------------------------------------------
GOOD_KEY = {"gamma": 2, "normalise": "focal", "class_weights": "median", "boundary": {"weight": 3.0, "sigma": 2.0, "radius": 4}}
BAD_KEYS = [({"gama": 2}, "gama"), ({"gamma": 0.5}, "gamma"), ({"normalise": "area"}, "normalise"),
            ({"class_weights": "frequency"}, "class_weights"), ({"class_weights": [1.0]}, "class_weights"),
            ({"boundary": {"weight": 1.0, "sigma": 1.0, "radius": 40}}, "radius"), ({"boundary": [1, 2, 3]}, "boundary"),
            ([("gamma", 2)], "mapping"), ("focal", "mapping"), (2, "mapping"), ({"gamma": 2, "smoothing": 0.1, "eps": 1}, "smoothing")]


def test_train_loss_key():
    from gan_segmentation_amd import main as cli
    assert cli.check_train_loss(None) is None
    assert cli.check_train_loss({}).as_dict() == LossSpec().as_dict()
    spec = cli.check_train_loss(GOOD_KEY)
    assert isinstance(spec, LossSpec) and spec.gamma == 2.0 and spec.normalise == "focal" and spec.needs_masks
    assert spec.boundary == {"weight": 3.0, "sigma": 2.0, "radius": 4}
    assert cli.check_train_loss({"class_weights": [1, 2.5]}).class_weights == (1.0, 2.5)
    for bad, word in BAD_KEYS:
        with pytest.raises(ValueError) as e:
            cli.check_train_loss(bad)
        assert "TRAIN_LOSS" in str(e.value) and word in str(e.value), (bad, str(e.value))


def test_train_reads_the_key_before_a_model_is_loaded(tmp_path):
    """A bad TRAIN_LOSS ends `train` with its message before anything touches BASE_DIR or a device; no key, no check."""
    from gan_segmentation_amd import main as cli
    cfg = {"BASE_DIR": str(tmp_path / "nowhere"), "GAN": "ffhq", "GAN_GPU_IDS": [0], "TRAIN_LOSS": {"normalise": "sum"}}
    with pytest.raises(ValueError) as e:
        cli.train(cfg)
    assert "TRAIN_LOSS" in str(e.value) and "normalise" in str(e.value)
    assert "TRAIN_LOSS" in cli.__doc__


def test_fit_checks_its_loss_before_reading_a_sample(tmp_path):
    """fit(loss=...) validates on entry: on a solver that has no device and no data behind it the error is the spec's."""
    from gan_segmentation_amd.seg_solver import SegSolver
    solver = object.__new__(SegSolver)
    solver.cfg = {"num_classes": 2}
    solver.path_to_data = str(tmp_path / "missing")
    for bad, word in BAD_KEYS:
        with pytest.raises(ValueError) as e:
            solver.fit(loss=bad)
        assert str(e.value).startswith("loss") and word in str(e.value), (bad, str(e.value))
    with pytest.raises(ValueError) as e:
        solver.fit(loss=LossSpec(class_weights=[1.0, 2.0, 3.0]))       # three weights for two classes
    assert "class_weights" in str(e.value) and "2" in str(e.value)
    with pytest.raises(FileNotFoundError):                             # a good spec gets as far as the data directory
        solver.fit(loss=dict(GOOD_KEY))


def test_defaults_are_none():
    from gan_segmentation_amd.seg_solver import SegSolver
    from gan_segmentation_amd.trainer import DecoderTrainer
    assert inspect.signature(DecoderTrainer.__init__).parameters["loss"].default is None
    assert inspect.signature(SegSolver.fit).parameters["loss"].default is None
    p = inspect.signature(loss_ops.softmax_loss).parameters
    assert p["spec"].default is None and p["grad"].default is True and p["dist2"].default is None and p["table"].default is None


def test_softmax_loss_refuses_host_tensors():
    import torch
    with pytest.raises(ValueError):
        loss_ops.softmax_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int8))


# ---- class weights from masks -------------------------------------------------------------------------------------------------
def _rows_of(masks):
    """pair_stats rows that hold the counts of ``masks`` (labels; everything outside 0..7 in slot 8) and nothing else."""
    rows = np.zeros((len(masks), pair_stats.ROW), np.int64)
    first = pair_stats.FIELDS["count"][0]
    for r, m in zip(rows, masks):
        slots = np.where((m >= 0) & (m < 8), m, 8).reshape(-1)
        r[first:first + pair_stats.SLOTS] = np.bincount(slots, minlength=pair_stats.SLOTS)
    return rows


@pytest.mark.parametrize("num_classes", [2, 3, 5, 8])
def test_class_weights_from_masks_are_those_of_summarise(num_classes):
    rng = np.random.default_rng(num_classes)
    H, W = 12, 20
    masks = []
    for i in range(6):
        m = rng.integers(-1, num_classes, (H, W)).astype(np.int32)
        m[rng.random((H, W)) < 0.5] = 0                 # class 0 dominates
        if i % 2:
            m[m == 1] = 0                               # class 1 is in every other sample only: presence matters
        if num_classes >= 5:
            m[m == 3] = 2                               # class 3 is absent everywhere
        masks.append(m)
    summary = pair_stats.summarise(list(range(6)), _rows_of(masks), H, W, 0, num_classes=num_classes)
    for scheme, key in (("median", "weights_median_frequency"), ("inverse", "weights_inverse_frequency")):
        got = loss_ops.class_weights_from_masks(masks, num_classes, scheme)
        assert got == summary[key][:num_classes], scheme              # the same floats, None where summarise has None
        assert len(got) == num_classes
    if num_classes >= 5:
        assert loss_ops.class_weights_from_masks(masks, num_classes)[3] is None
    assert loss_ops.class_weights_from_masks(masks, num_classes) == loss_ops.class_weights_from_masks(masks, num_classes, "median")
    assert loss_ops.class_weights_from_masks(iter(masks), num_classes, "inverse")[0] < 1.0       # the dominant class weighs least


def test_class_weights_from_masks_beyond_the_slots_of_pair_stats():
    """More than 8 classes: the helper is not bound to pair_stats' nine slots."""
    m = np.arange(12 * 12).reshape(12, 12) % 12
    got = loss_ops.class_weights_from_masks([m, m], 12, "inverse")
    assert got == pytest.approx([1.0] * 12) and loss_ops.class_weights_from_masks([m], 12, "median") == [1.0] * 12


def test_class_weights_from_masks_rejects():
    m = np.zeros((4, 4), np.int32)
    for args in (([], 2), ([m, np.zeros((4, 5), np.int32)], 2), ([m.astype(np.float32)], 2), ([m], 1), ([m], 65), ([m], 2.0),
                 ([m], 2, "mean")):
        with pytest.raises(ValueError):
            loss_ops.class_weights_from_masks(*args)
    assert loss_ops.class_weights_from_masks([np.full((4, 4), -1)], 2) == [None, None]
