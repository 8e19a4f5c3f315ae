"""Weights of a learned super-resolution model for Encoder.set_sr_model: an RRDBNet state dict, as the RealESRGAN project publishes
RealESRGAN_x4plus, RealESRGAN_x2plus and RealESRGANv2-anime_6B, or an SRVGGNetCompact one (§6m: realesr-animevideov3, realesr-general-x4v3 and its denoise
partner realesr-general-wdn-x4v3), read with torch and flattened into the order hevc_amd/csrc/sr_net.h / sr_compact_net.h states.  load_model chooses by the
keys; load_rrdbnet refuses compact models by name and load_compact everything else.  blend is the compact family's denoise strength.  No weights ship with
the package.  Not covered: scale 1 and 3 models, num_feat / num_grow_ch other than 64 / 32."""
import re
from dataclasses import dataclass

import numpy as np


@dataclass
class RrdbNet:
    scale: int             # 4 or 2
    blocks: int            # RRDBs in the trunk
    weights: np.ndarray    # float32, flat: per layer the weight [cout][cin][3][3], then the bias

    def __repr__(self):
        return f"RrdbNet(scale={self.scale}, blocks={self.blocks}, {self.weights.size} weights)"


def layer_names(blocks: int):
    """the layers in the flat order"""
    return (["conv_first"] + [f"body.{i}.rdb{r}.conv{k}" for i in range(blocks) for r in (1, 2, 3) for k in (1, 2, 3, 4, 5)]
            + ["conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"])


def _shape(name: str, cin_first: int):
    if name == "conv_first":
        return 64, cin_first
    if name == "conv_last":
        return 3, 64
    if ".conv" in name:
        k = int(name[-1])
        return (64 if k == 5 else 32), 64 + 32 * (k - 1)
    return 64, 64


def load_rrdbnet(source) -> RrdbNet:
    """source: the path of a .pth file, or a state dict (name -> tensor or array), bare or under 'params_ema' / 'params'.  Raises ValueError, naming the key, for
    anything that is not an RRDBNet of 64 features and 32 growth channels with 3 (scale 4) or 12 (scale 2) input channels"""
    if not isinstance(source, dict):
        import importlib
        torch = importlib.import_module("torch")      # only here: the package itself runs without torch, a .pth file cannot be read without it
        source = torch.load(str(source), map_location="cpu", weights_only=True)
        if not isinstance(source, dict):
            raise ValueError("not a state dict")
    for wrap in ("params_ema", "params"):
        if wrap in source and isinstance(source[wrap], dict):
            source = source[wrap]
            break
    sd = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in source.items()}
    if any(k.startswith("body.") and ".rdb" not in k for k in sd) or "conv_first.weight" not in sd:
        raise ValueError("not an RRDBNet state dict (an SRVGGNetCompact model such as realesr-general is not covered): keys " + ", ".join(sorted(sd)[:4]) + " ...")
    ids = {int(m.group(1)) for k in sd for m in [re.match(r"body\.(\d+)\.rdb", k)] if m}
    blocks = len(ids)
    if blocks < 1 or ids != set(range(blocks)):
        raise ValueError(f"body blocks {sorted(ids)} are not 0 .. n - 1")
    first = sd["conv_first.weight"]
    if first.ndim != 4 or first.shape[1] not in (3, 12):
        raise ValueError(f"conv_first.weight has shape {tuple(first.shape)}: 3 input channels (scale 4) or 12 (scale 2) are covered, scale 1 models (48) are not")
    scale = 4 if first.shape[1] == 3 else 2
    names = layer_names(blocks)
    known = {n + s for n in names for s in (".weight", ".bias")}
    extra = sorted(set(sd) - known)
    if extra:
        raise ValueError(f"unexpected key {extra[0]}")
    parts = []
    for n in names:
        cout, cin = _shape(n, int(first.shape[1]))
        for suffix, shape in ((".weight", (cout, cin, 3, 3)), (".bias", (cout,))):
            if n + suffix not in sd:
                raise ValueError(f"missing key {n + suffix}")
            a = sd[n + suffix]
            if tuple(a.shape) != shape:
                raise ValueError(f"{n + suffix} has shape {tuple(a.shape)}, not {shape}: num_feat 64 and num_grow_ch 32 are what is covered")
            parts.append(np.asarray(a, np.float32).reshape(-1))
    return RrdbNet(scale, blocks, np.concatenate(parts))


@dataclass
class CompactNet:
    scale: int             # 4 or 2
    convs: int             # trunk convolutions (16 in realesr-animevideov3, 32 in realesr-general-x4v3)
    weights: np.ndarray    # float32, flat, the state dict's order: per layer the weight [cout][cin][3][3], the bias, and (all but the last) the PReLU slopes [64]

    def __repr__(self):
        return f"CompactNet(scale={self.scale}, convs={self.convs}, {self.weights.size} weights)"


def compact_count(scale: int, convs: int) -> int:
    """floats of the flat weights (sr_compact_net.h, sr_compact_count)"""
    return 64 * 27 + 128 + convs * (64 * 576 + 128) + 3 * scale * scale * 577


def _state_dict(source):
    if not isinstance(source, dict):
        import importlib
        torch = importlib.import_module("torch")      # only here: the package itself runs without torch, a .pth file cannot be read without it
        source = torch.load(str(source), map_location="cpu", weights_only=True)
        if not isinstance(source, dict):
            raise ValueError("not a state dict")
    for wrap in ("params_ema", "params"):
        if wrap in source and isinstance(source[wrap], dict):
            source = source[wrap]
            break
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in source.items()}


def load_compact(source) -> CompactNet:
    """source: the path of a .pth file, or a state dict (name -> tensor or array), bare or under 'params_ema' / 'params'.  Raises ValueError, naming the key, for
    anything that is not an SRVGGNetCompact of 64 features with per-channel PReLU, 3 input channels and 48 (scale 4) or 12 (scale 2) output channels:
    body.0 is the first convolution, body.1 its slopes, body.2 k / body.2 k + 1 trunk layer k - 1, and the last even index the last convolution"""
    sd = _state_dict(source)
    if "body.0.weight" not in sd or any(not re.fullmatch(r"body\.\d+\.(weight|bias)", k) for k in sd):
        bad = next((k for k in sorted(sd) if not re.fullmatch(r"body\.\d+\.(weight|bias)", k)), "body.0.weight")
        raise ValueError(f"not an SRVGGNetCompact state dict: key {bad}" + (" (an RRDBNet: load_rrdbnet)" if "conv_first.weight" in sd else ""))
    ids = sorted({int(k.split(".")[1]) for k in sd})
    last = ids[-1]
    if ids != list(range(last + 1)) or last % 2 or last < 4:
        raise ValueError(f"body entries {ids[:3]} .. {last} are not convolutions and activations in turn with a last convolution: key body.{last}.weight")
    convs = last // 2 - 1
    if convs > 64:
        raise ValueError(f"body.{last}.weight: {convs} trunk convolutions, 1 .. 64 are covered")
    tail = sd.get(f"body.{last}.weight")
    if tail is None or tail.ndim != 4 or tail.shape[0] not in (48, 12):
        shape = None if tail is None else tuple(tail.shape)
        raise ValueError(f"body.{last}.weight has shape {shape}: 48 output channels (scale 4) or 12 (scale 2) are covered, scale 3 (27) and scale 1 (3) are not")
    scale = 4 if tail.shape[0] == 48 else 2
    parts = []
    for i in ids:
        if i % 2:
            want = {".weight": (64,)}
        else:
            cout, cin = (3 * scale * scale if i == last else 64), (3 if i == 0 else 64)
            want = {".weight": (cout, cin, 3, 3), ".bias": (cout,)}
        extra = sorted(k for k in sd if k.startswith(f"body.{i}.") and k[len(f"body.{i}"):] not in want)
        if extra:
            raise ValueError(f"unexpected key {extra[0]}")
        for suffix, shape in want.items():
            k = f"body.{i}{suffix}"
            if k not in sd:
                raise ValueError(f"missing key {k}")
            if tuple(sd[k].shape) != shape:
                raise ValueError(f"{k} has shape {tuple(sd[k].shape)}, not {shape}: num_feat 64, 3 input channels and one PReLU slope per channel are what is covered")
            parts.append(np.asarray(sd[k], np.float32).reshape(-1))
    return CompactNet(scale, convs, np.concatenate(parts))


def load_model(source):
    """load_rrdbnet or load_compact, chosen by the keys: a state dict with body.0.weight is an SRVGGNetCompact, anything else goes to load_rrdbnet (whose
    errors name the key)"""
    sd = _state_dict(source)
    return load_compact(sd) if "body.0.weight" in sd else load_rrdbnet(sd)


def blend(a: CompactNet, b: CompactNet, strength: float) -> CompactNet:
    """The compact family's denoise strength (realesr-general-x4v3 with realesr-general-wdn-x4v3): every parameter is strength a + (1 - strength) b, in
    float32, strength in [0, 1].  0 and 1 return b and a themselves.  Models of different shapes are refused"""
    if not isinstance(a, CompactNet) or not isinstance(b, CompactNet):
        raise ValueError("blend takes two CompactNet models (an RRDBNet has no denoise partner)")
    if (a.scale, a.convs, a.weights.shape) != (b.scale, b.convs, b.weights.shape):
        raise ValueError(f"blend of models of different shapes: {a!r} and {b!r}")
    strength = float(strength)
    if not 0.0 <= strength <= 1.0:      # (NaN too)
        raise ValueError(f"blend strength {strength} is outside [0, 1]")
    if strength == 1.0:
        return a
    if strength == 0.0:
        return b
    s = np.float32(strength)
    return CompactNet(a.scale, a.convs, s * a.weights.astype(np.float32) + (np.float32(1.0) - s) * b.weights.astype(np.float32))
