"""CPU: hevc_amd.sr for compact models: load_compact and load_model over synthetic state dicts (arrays, tensors, a .pth file, bare and wrapped), blend, and
the errors, which name the key.  No weights ship: the state dicts are random."""
import numpy as np
import pytest

from hevc_amd import sr
from tests import sr_compact_ref as R
from tests import sr_ref


def compact_dict(scale=4, convs=2, seed=1):
    return R.random_weights(scale, convs, seed)


@pytest.mark.parametrize("scale,convs", [(4, 1), (4, 16), (2, 3), (2, 32)])
def test_a_compact_state_dict_round_trips(scale, convs):
    w = compact_dict(scale, convs)
    for source in (w, {"params": w}, {"params_ema": dict(reversed(list(w.items())))}):
        for load in (sr.load_compact, sr.load_model):
            m = load(source)
            assert isinstance(m, sr.CompactNet) and (m.scale, m.convs) == (scale, convs)
            assert m.weights.dtype == np.float32 and m.weights.size == sr.compact_count(scale, convs) == R.count(scale, convs)
            assert np.array_equal(m.weights, R.flatten(w, convs))


def test_an_rrdbnet_state_dict_round_trips_through_load_model():
    w = sr_ref.random_weights(4, 1, 3)
    m = sr.load_model({"params_ema": w})
    assert isinstance(m, sr.RrdbNet) and (m.scale, m.blocks) == (4, 1) and np.array_equal(m.weights, sr_ref.flatten(w, 1))


def test_tensors_and_a_pth_file(tmp_path):
    import torch
    w = compact_dict(2, 2)
    t = {k: torch.from_numpy(v) for k, v in w.items()}
    assert np.array_equal(sr.load_model(t).weights, R.flatten(w, 2))
    torch.save({"params": t}, tmp_path / "compact.pth")
    m = sr.load_model(tmp_path / "compact.pth")
    assert (m.scale, m.convs) == (2, 2) and np.array_equal(m.weights, R.flatten(w, 2))
    assert np.array_equal(sr.load_compact(str(tmp_path / "compact.pth")).weights, m.weights)


def test_blend():
    a, b = sr.load_compact(compact_dict(4, 2, 1)), sr.load_compact(compact_dict(4, 2, 2))
    assert sr.blend(a, b, 1) is a and sr.blend(a, b, 0.0) is b
    half = sr.blend(a, b, 0.5)
    assert (half.scale, half.convs) == (4, 2) and half.weights.dtype == np.float32
    assert np.array_equal(half.weights, (a.weights + b.weights) * np.float32(0.5))          # (halving is exact, so the mean in float32)
    q = sr.blend(a, b, 0.25)
    assert np.array_equal(q.weights, np.float32(0.25) * a.weights + np.float32(0.75) * b.weights)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            sr.blend(a, b, bad)
    with pytest.raises(ValueError, match="different shapes"):
        sr.blend(a, sr.load_compact(compact_dict(4, 3)), 0.5)
    with pytest.raises(ValueError, match="different shapes"):
        sr.blend(a, sr.load_compact(compact_dict(2, 2)), 0.5)
    with pytest.raises(ValueError, match="CompactNet"):
        sr.blend(a, sr.load_rrdbnet(sr_ref.random_weights(4, 1, 3)), 0.5)


def test_errors_name_the_key():
    w = compact_dict(4, 2)
    last = "body.6.weight"
    cases = [
        ({k: v for k, v in w.items() if k != "body.2.bias"}, "missing key body.2.bias"),
        ({**w, "body.3.bias": np.zeros(64, np.float32)}, "unexpected key body.3.bias"),
        ({**w, "body.3.weight": np.zeros(1, np.float32)}, r"body.3.weight has shape \(1,\)"),
        ({**w, "body.2.weight": np.zeros((64, 32, 3, 3), np.float32)}, r"body.2.weight has shape \(64, 32, 3, 3\)"),
        ({**w, last: np.zeros((27, 64, 3, 3), np.float32)}, r"body.6.weight has shape \(27, 64, 3, 3\)"),
        ({**w, last: np.zeros((3, 64, 3, 3), np.float32)}, r"body.6.weight has shape \(3, 64, 3, 3\)"),
        ({**w, "upsampler.weight": np.zeros(1, np.float32)}, "key upsampler.weight"),
        ({k: v for k, v in w.items() if not k.startswith("body.4.")}, "body.6.weight"),
        ({k: v for k, v in w.items() if not k.startswith("body.6.")}, "body.5.weight"),
    ]
    for source, pattern in cases:
        for load in (sr.load_compact, sr.load_model):
            with pytest.raises(ValueError, match=pattern):
                load(source)
    with pytest.raises(ValueError, match="RRDBNet"):
        sr.load_compact(sr_ref.random_weights(4, 1, 3))
    with pytest.raises(ValueError, match="SRVGGNetCompact"):          # load_rrdbnet keeps refusing compact models by name
        sr.load_rrdbnet(w)
    with pytest.raises(ValueError, match="conv_first|keys"):          # neither kind: load_rrdbnet's error
        sr.load_model({"foo.weight": np.zeros(1, np.float32)})
