"""CPU: hevc_amd.sr.load_rrdbnet reads an RRDBNet state dict (bare, under 'params_ema', under 'params', from a .pth file) into the flat order of
hevc_amd/csrc/sr_net.h, infers blocks and scale, and refuses everything else by name; encode_file(sr_model=) refuses what it cannot combine before a session
exists."""
import numpy as np
import pytest

from hevc_amd import sr
from tests import sr_ref as R


def state_dict(scale, blocks, seed=1):
    import torch
    return {k: torch.from_numpy(v) for k, v in R.random_weights(scale, blocks, seed).items()}


@pytest.mark.parametrize("scale,blocks", [(4, 1), (2, 2), (4, 6)])
@pytest.mark.parametrize("wrap", [None, "params_ema", "params"])
def test_round_trip_through_a_pth_file(tmp_path, scale, blocks, wrap):
    import torch
    sd = state_dict(scale, blocks)
    path = tmp_path / "model.pth"
    torch.save({wrap: sd, "other": 1} if wrap else sd, path)
    for source in (path, {wrap: sd} if wrap else sd):
        m = sr.load_rrdbnet(source)
        assert (m.scale, m.blocks) == (scale, blocks) and m.weights.dtype == np.float32
        want = R.flatten({k: v.numpy() for k, v in sd.items()}, blocks)
        assert m.weights.size == want.size == sum(v.numel() for v in sd.values()) and np.array_equal(m.weights, want)
    # the flat order: conv_first's weight, its bias, then body.0.rdb1.conv1
    assert np.array_equal(m.weights[:sd["conv_first.weight"].numel()], sd["conv_first.weight"].numpy().reshape(-1))
    assert sr.layer_names(blocks) == R.layer_names(blocks)


def test_params_ema_wins_over_params():
    a, b = state_dict(4, 1, 1), state_dict(4, 1, 2)
    assert np.array_equal(sr.load_rrdbnet({"params": a, "params_ema": b}).weights, sr.load_rrdbnet(b).weights)


def test_refusals_name_the_key():
    import torch
    sd = state_dict(4, 1)
    bad = dict(sd)
    bad["body.0.rdb2.conv3.weight"] = torch.zeros(32, 128, 3, 3)[:, :96]          # a wrong feature count
    with pytest.raises(ValueError, match="body.0.rdb2.conv3.weight"):
        sr.load_rrdbnet(bad)
    bad = {k: v for k, v in sd.items() if k != "conv_hr.bias"}
    with pytest.raises(ValueError, match="missing key conv_hr.bias"):
        sr.load_rrdbnet(bad)
    bad = dict(sd)
    bad["conv_first.weight"] = torch.zeros(64, 48, 3, 3)                            # a scale 1 model: 48 input channels
    with pytest.raises(ValueError, match="48"):
        sr.load_rrdbnet(bad)
    bad = dict(sd)
    bad["conv_extra.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="conv_extra.weight"):
        sr.load_rrdbnet(bad)
    with pytest.raises(ValueError, match="SRVGGNetCompact"):
        sr.load_rrdbnet({"body.0.weight": torch.zeros(64, 3, 3, 3), "body.0.bias": torch.zeros(64)})
    bad = {k: v for k, v in state_dict(4, 2).items() if not k.startswith("body.0.")}
    with pytest.raises(ValueError, match="blocks"):
        sr.load_rrdbnet(bad)


def test_encode_file_refuses_combinations_and_bad_models_before_a_session(tmp_path, monkeypatch):
    from hevc_amd import encoder
    from tests.ingest_common import info
    made = []
    monkeypatch.setattr(encoder, "Encoder", lambda *a, **k: made.append(1))
    model = sr.load_rrdbnet(state_dict(2, 1))
    src = info("gbrp", 64, 48, 3)
    for kw in (dict(size=(128, 96)), dict(upscale=(128, 96)), dict(deinterlace="frame"), dict(denoise=2), dict(lut="hdr-to-sdr"), dict(interpolate=2),
               dict(devices=[0, 1])):
        assert encoder.encode_file(tmp_path / "a.mov", tmp_path / "o.mp4", src, total_frames=3, sr_model=model, **kw) == 1, kw
    assert encoder.encode_file(tmp_path / "a.mov", tmp_path / "o.mp4", src, total_frames=3, sr_model=tmp_path / "none.pth") == 1
    assert encoder.encode_file(tmp_path / "a.mov", tmp_path / "o.mp4", info("gbrp", 63, 48, 3), total_frames=3, sr_model=model) == 1      # odd with scale 2
    assert not made
