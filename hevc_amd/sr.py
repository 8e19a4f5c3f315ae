"""Weights of a learned super-resolution model for Encoder.set_sr_model: an RRDBNet state dict, as the RealESRGAN project publishes
RealESRGAN_x4plus, RealESRGAN_x2plus and RealESRGANv2-anime_6B, read with torch and flattened into the order hevc_amd/csrc/sr_net.h states.  No weights ship
with the package.  Not covered, and refused by name: SRVGGNetCompact models (realesr-general, realesr-animevideov3), scale 1 models, num_feat / num_grow_ch
other than 64 / 32."""
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
