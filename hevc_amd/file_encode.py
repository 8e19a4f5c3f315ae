"""One file through the native MI355X encoder: `encode_file` is what `convert_video` calls for the 'MI355X' backend: probe -> operating point (the same numbers
the reference hands to libx265, core/transcoder.py:357-412) -> read frames -> session -> Annex-B packets -> MP4 (hvc1).

A run is planned before anything is opened: `_plan_options` judges the options and the probe, `_plan_clip` adds what only the opened clip can say, and the
`_Plan` names the description the session is derived from, its set-up calls and ONE sender for every frame; one loop then runs every plan.  The sessions and
config_for live in hevc_amd.encoder, which re-exports this module's public names, and are looked up there when they are called (the tests put stand-ins there).
"""
from __future__ import annotations

import contextlib
import copy
import functools
import itertools
import logging
import threading
from dataclasses import dataclass, replace
from fractions import Fraction
from pathlib import Path
from typing import Callable, Optional, Tuple

from . import _lib
from .probe import VideoInfo

logger = logging.getLogger(__name__)


def upscale_target(w: int, h: int, target_height: int = 0) -> Tuple[int, int]:
    """The size the reference's upscaling tool gives a w x h clip: target_height 0 picks 1080 lines below 1080, 2160 below 2160, else the source's own height; a
    non-zero target_height is taken as given.  scale = target_height / h and width = int(w * scale), in its floating-point arithmetic, the width then lowered to
    the next even number (4:2:0)."""
    if target_height == 0:
        target_height = 1080 if h < 1080 else 2160 if h < 2160 else h
    scale = target_height / h
    return int(w * scale) & ~1, int(target_height)


def sr_target_size(sw: int, sh: int, scale: int, target=None) -> Tuple[int, int]:
    """The session size of a sw x sh source through a model of `scale` (Encoder.send_sr_yuv, Encoder.send_sr_fit).  target None: the network's own output,
    (scale sw, scale sh).  'auto': upscale_target(sw, sh, 0), the reference's rule (1080 lines for sources below 1080, 2160 below 2160); an int: that height,
    upscale_target(sw, sh, height); a (w, h) tuple is taken as given.  The result must be the network's output size, or a reduction of it the device scaler
    takes: all sizes even and at least 16, per axis between a quarter of the network's output and that output.  ValueError names the sizes otherwise; a target
    LARGER than the network's output (a 240-line source to 1080 through a x4 model) is one of them."""
    sw, sh, scale = int(sw), int(sh), int(scale)
    nw, nh = scale * sw, scale * sh
    if target is None:
        return nw, nh
    if isinstance(target, str):
        if target != 'auto':
            raise ValueError(f"sr_target={target!r} takes (w, h), a height or 'auto'")
        w, h = upscale_target(sw, sh, 0)
    elif isinstance(target, int) and not isinstance(target, bool):
        if target < 1:
            raise ValueError(f"sr_target={target!r} takes (w, h), a height or 'auto'")
        w, h = upscale_target(sw, sh, target)
    else:
        try:
            w, h = (int(x) for x in target)
        except (TypeError, ValueError):
            raise ValueError(f"sr_target={target!r} takes (w, h), a height or 'auto'") from None
    if (w, h) == (nw, nh):
        return w, h
    if any(x % 2 or x < 16 for x in (w, h, nw, nh)) or not nw <= 4 * w <= 4 * nw or not nh <= 4 * h <= 4 * nh:
        raise ValueError(f"a {sw}x{sh} source through a x{scale} model is {nw}x{nh}: {w}x{h} is not that size or an even reduction of it by at most 4 per axis")
    return w, h


def remux_audio(video_mp4: Path, source: Path, out_path: Path, info: VideoInfo) -> bool:
    """The native path writes video only; the reference always carries the source's audio as AAC (core/transcoder.py:423-450,480-489).
    When the source has audio (only container inputs can, and those need ffmpeg to be decoded at all) the video track is copied and the
    audio encoded with the reference's own flags.  False when ffmpeg is missing or fails: the caller then falls down the ladder."""
    import shutil
    import subprocess
    from .transcoder import VIDEO_METADATA_FLAGS, get_audio_flags
    if shutil.which('ffmpeg') is None:
        return False
    cmd = ['ffmpeg', '-hide_banner', '-y', '-i', str(video_mp4), '-i', str(source), '-map', '0:v:0', '-map', '1:a:0?', '-map_metadata', '1',
           '-c:v', 'copy', '-tag:v', 'hvc1'] + VIDEO_METADATA_FLAGS
    for kv in ('handler_name=SoundHandler', f'language={info.audio_language or "eng"}', 'title="Main Audio"'):
        cmd += ['-metadata:s:a:0', kv]
    cmd += get_audio_flags(info.audio_channels) + ['-brand', 'mp42', '-movflags', '+write_colr+use_metadata_tags+faststart', str(out_path)]
    try:
        return subprocess.run(cmd, capture_output=True).returncode == 0 and Path(out_path).exists()
    except Exception:
        return False


def _parse_upscale(upscale, sw: int, sh: int) -> Tuple[int, int]:
    """upscale= of encode_file: (w, h), a target height, or 'auto' for upscale_target's rule -> the target size.  ValueError / TypeError / IndexError otherwise"""
    if isinstance(upscale, str):
        if upscale != 'auto':
            raise ValueError(upscale)
        return upscale_target(sw, sh, 0)
    if isinstance(upscale, int) and not isinstance(upscale, bool):
        if upscale < 1:
            raise ValueError(upscale)
        return upscale_target(sw, sh, upscale)
    target = (int(upscale[0]), int(upscale[1]))
    if len(upscale) != 2:
        raise ValueError(upscale)
    return target


def _load_sr(sr_model, sr_denoise):
    """sr_model= / sr_denoise= of encode_file -> an hevc_amd.sr.RrdbNet or CompactNet: a model as it is, a path or state dict loaded, a pair blended by
    sr_denoise.  Raises what the loaders raise, and ValueError for a pair without its strength or a strength without its pair"""
    from . import sr as sr_mod
    one = lambda m: m if isinstance(m, (sr_mod.RrdbNet, sr_mod.CompactNet)) else sr_mod.load_model(m)
    if isinstance(sr_model, (tuple, list)):
        if len(sr_model) != 2 or sr_denoise is None or isinstance(sr_denoise, bool):
            raise ValueError("a pair (model, denoise partner) goes with sr_denoise = 0 .. 1")
        return sr_mod.blend(one(sr_model[0]), one(sr_model[1]), sr_denoise)
    if sr_denoise is not None:
        raise ValueError("sr_denoise= goes with a pair (model, denoise partner) of compact models")
    return one(sr_model)


def _field_order(file_path: Path, tff, deinterlace: str):
    """the field order of deinterlace=: tff when given, else the y4m header's It / Ib tag or ffprobe's field_order; a source that names none is top field first,
    but for 'auto', which then does nothing (None)"""
    from . import yuvio
    order = tff
    if order is None:
        suffix = Path(file_path).suffix.lower()
        if suffix == '.y4m':
            probe_clip = yuvio.open_clip(Path(file_path))
            order = {'t': True, 'b': False}.get(probe_clip.interlace)
            probe_clip.close()
        elif suffix != '.yuv':
            from .probe import probe_field_order
            order = probe_field_order(Path(file_path))
        if order is None and deinterlace != 'auto':
            order = True
    return order


def _sr_source_colour(info: VideoInfo, clip, height: int):
    """(matrix, full range) of a Y'CbCr source on its way into the network: the probed matrix, BT.601 below 720 lines and BT.709 from there on when the probe does
    not know it; yuvj* files read directly are full range (the pipe hands yuvj* over as limited range)"""
    from . import encoder as _enc, yuvio
    matrix = _enc._COLOUR_CODES["matrix"].get(info.color_space, 0)
    if matrix not in (1, 5, 6, 9):
        matrix = 6 if height < 720 else 1
    return matrix, (info.pix_fmt or '').lower().startswith('yuvj') and not isinstance(clip, yuvio._PipeClip)


def _carry_audio(wants_audio: bool, video_path: Path, file_path: Path, out_path: Path, info: VideoInfo) -> bool:
    """the end of an encode, the video track written: a source with audio gets its audio carried over.  False: the remux failed"""
    if not wants_audio:
        return True
    good = remux_audio(video_path, Path(file_path), Path(out_path), info)
    try:
        video_path.unlink()
    except OSError:
        pass
    if not good:
        logger.warning("%s: audio could not be carried over (ffmpeg remux failed); falling back to the ffmpeg path", Path(file_path).name)
    return good


CHAIN_KEYS = ("deinterlace", "tff", "denoise", "size", "upscale", "sr_model", "sr_target", "sr_denoise", "sharpen", "antiring", "interpolate", "interp_mode")

# Which source options of encode_file go together: every pair that is not named here is refused, in one place (_refuse_pairs).  No two of the seven filters go
# together and none runs over several devices; native_rgb only says how an RGB container is read: size= judges that by the clip, sr_model= decides it for itself.
_OPTIONS = ("denoise", "upscale", "sr_model", "interpolate", "lut", "deinterlace", "size", "native_rgb", "devices", "row_split")
_TOGETHER = {frozenset(p) for p in (("size", "native_rgb"), ("sr_model", "native_rgb"), ("native_rgb", "devices"), ("native_rgb", "row_split"), ("devices", "row_split"))}
_SPELLING = {"native_rgb": "native_rgb", "devices": "several devices", "row_split": "row_split"}      # the others are keywords: name=


class _Refused(Exception):
    """what encode_file does not take, worded for the log: the run ends with 1 before a session exists"""


def _refuse_pairs(on):
    spell = lambda k: _SPELLING.get(k, k + "=")
    for a, b in itertools.combinations([k for k in _OPTIONS if k in on], 2):
        if frozenset((a, b)) not in _TOGETHER:
            partners = [spell(k) for k in _OPTIONS if frozenset((a, k)) in _TOGETHER]
            raise _Refused(f"{spell(a)} does not go with {spell(b)}: beside it there may be {', '.join(partners) if partners else 'no other source option'}")


@dataclass(frozen=True)
class _Plan:
    """What the run of encode_file needs, and nothing else"""
    clip_info: VideoInfo                            # what the clip is opened with: the source's own description, size, rate and frame count
    info: VideoInfo                                 # what the session, its level and the MP4 track are derived from
    open_flags: dict                                # of yuvio.open_any
    rate: Optional[Fraction] = None                 # the session's rate where info.fps cannot say it: an exact fraction
    count: Callable[[int], int] = int               # frames of the source -> pictures of the session (the progress total)
    setup: tuple = ()                               # (method of the session, arguments) to call before the first frame
    matrix: int = 0                                 # what the session signals where the probe names no matrix the device converts to (0: nothing to say)
    own_depth: bool = False                         # the session's depth is the option's: the depth in the clip's header does not outrank the probe
    send: Optional[Callable] = None                 # (session, frame number, planes): the sender of every frame; None until the clip's format chooses it
    on_clip: Optional[Callable] = None              # (plan, clip) -> plan: the checks and choices that wait for the opened clip; raises _Refused


def _session_info(info: VideoInfo, size=None, rate=None, count=None, sdr_depth=None):
    """The description a session is derived from, made of the source's in one step -> (it, the exact rate).  size: the session's (w, h); rate: the factor on the
    source's rate, whose product is exact as a fraction (the second result; None where the float says it: a whole factor); count: frames -> pictures; sdr_depth:
    the rewrite of lut=: an SDR clip of that depth whatever the probe says."""
    out, exact = copy.copy(info), None
    if size is not None:
        out.width, out.height = int(size[0]), int(size[1])
    if rate is not None:
        rate = Fraction(rate)
        exact = Fraction(str(info.fps or 30.0)).limit_denominator(1001) * rate
        out.fps = float(info.fps or 30.0) * float(rate) if rate.denominator == 1 else float(exact)
        exact = None if rate.denominator == 1 else exact
    if count is not None:
        out.nb_frames = max(int(count(int(getattr(info, 'nb_frames', 0) or 0))), 0)
    if sdr_depth is not None:
        out.hdr, out.master_display, out.max_cll = False, '', ''
        out.color_primaries = out.color_transfer = out.color_space = 'bt709'
        out.pix_fmt = 'yuv420p10le' if sdr_depth == 10 else 'yuv420p'
    return out, exact


def _layout(clip):
    """the clip's sample layout where it is not the session's own: its RgbFormat or SrcFormat, else None"""
    return getattr(clip, 'rgb_format', None) or getattr(clip, 'src_format', None)


def _sample_depth(clip) -> int:
    fmt = getattr(clip, 'src_format', None)
    return int(fmt.bit_depth) if fmt is not None else int(clip.bit_depth)


def _planar420(clip, depths=None) -> bool:
    """Whether the clip's frames are planar 4:2:0 in the session's element layout (not RGB, not semi-planar, not msb-aligned) at one of `depths` (None: any).
    At the depth of its own session, (clip.bit_depth,), that is the plain layout Encoder.send takes."""
    fmt = getattr(clip, 'src_format', None)
    planar = getattr(clip, 'rgb_format', None) is None and (fmt is None or (fmt.chroma == 420 and not fmt.semi_planar and not fmt.msb_aligned))
    return planar and (depths is None or _sample_depth(clip) in depths)


def _needs_plain_frames(option: str, height_multiple: int, send):
    """on_clip of the filters that run at the session's own size and depth: the check and then the sender"""
    def on_clip(plan, clip):
        w, h = int(plan.info.width), int(plan.info.height)
        if not _planar420(clip, (clip.bit_depth,)) or w % 2 or h % height_multiple or min(w, h) < 16:
            sides = "width and height even" if height_multiple == 2 else f"width even, height a multiple of {height_multiple}"
            raise _Refused(f"{option} takes a planar 4:2:0 source at the session's depth, {sides} ({_layout(clip)!r}, {w}x{h})")
        return replace(plan, send=send)
    return on_clip


def _resized(option: str, send_name: str, **kw):
    """on_clip of size= and upscale=: the clip delivers its own size and depth, the device brings it to the session's"""
    def on_clip(plan, clip):
        if not _planar420(clip):
            raise _Refused(f"{option} takes a planar 4:2:0 source on one device ({_layout(clip)!r})")
        w, h, depth = int(clip.width), int(clip.height), _sample_depth(clip)
        return replace(plan, send=lambda enc, i, planes: getattr(enc, send_name)(w, h, *planes, bit_depth=depth, pts=i, **kw))
    return on_clip


def _plan_chain(file_path, info, total_frames, chain) -> _Plan:
    """chain=: the options of the dict become one _lib.Chain, the session opens at what mihevc_chain_plan_for says of it, every frame goes through
    Encoder.send_chain"""
    if not isinstance(chain, dict) or set(chain) - set(CHAIN_KEYS):
        raise _Refused(f"chain= takes a dict with keys out of {', '.join(CHAIN_KEYS)}")
    opt = {k: chain.get(k) for k in CHAIN_KEYS}
    sw0, sh0 = int(info.width), int(info.height)
    kw = {}
    # field
    deinterlace = opt["deinterlace"]
    if deinterlace is not None:
        if deinterlace not in ('frame', 'field', 'auto', 'ivtc', 'match'):
            raise _Refused(f"chain: deinterlace={deinterlace!r} takes 'frame', 'field', 'auto', 'ivtc' or 'match'")
        order = _field_order(file_path, opt["tff"], deinterlace)
        if deinterlace in ('ivtc', 'match'):
            kw.update(field="fieldmatch", tff=bool(order), decimate=deinterlace == 'ivtc', fm_deint=True)
        elif order is not None:
            kw.update(field="deint", tff=bool(order), field_rate=deinterlace == 'field')
    elif opt["tff"] is not None:
        raise _Refused("chain: tff= goes with deinterlace=")
    # denoise
    dn = opt["denoise"]
    if dn is not None and not (isinstance(dn, int) and not isinstance(dn, bool) and dn == 0):
        try:
            kw["denoise"] = _lib.denoise_strength(dn)
        except (TypeError, ValueError):
            raise _Refused(f"chain: denoise={dn!r} takes a level 0 .. 3 or four thresholds 0 .. 255") from None
    # resize
    if sum(opt[k] is not None for k in ("size", "upscale", "sr_model")) > 1:
        raise _Refused("chain: one of size=, upscale=, sr_model=")
    target, sr = (sw0, sh0), None
    sharpen, antiring = (8 if opt[k] is None else opt[k] for k in ("sharpen", "antiring"))
    if opt["upscale"] is None and (opt["sharpen"] is not None or opt["antiring"] is not None):
        raise _Refused("chain: sharpen= and antiring= go with upscale=")
    if opt["sr_model"] is None and (opt["sr_target"] is not None or opt["sr_denoise"] is not None):
        raise _Refused("chain: sr_target= and sr_denoise= go with sr_model=")
    try:
        if opt["size"] is not None:
            target = (int(opt["size"][0]), int(opt["size"][1]))
            if len(opt["size"]) != 2:
                raise ValueError(opt["size"])
            kw["resize"] = "scale"
        elif opt["upscale"] is not None:
            if any(isinstance(x, bool) or not isinstance(x, int) for x in (sharpen, antiring)):
                raise ValueError("sharpen / antiring")
            target = _parse_upscale(opt["upscale"], sw0, sh0)
            kw.update(resize="upscale", sharpen=sharpen, antiring=antiring)
        elif opt["sr_model"] is not None:
            sr = _load_sr(opt["sr_model"], opt["sr_denoise"])
            target = sr_target_size(sw0, sh0, sr.scale, opt["sr_target"])
            kw["resize"] = "sr"
    except (OSError, ValueError, TypeError, RuntimeError, KeyError, IndexError) as e:
        raise _Refused(f"chain: the resize stage: {e}") from None
    # interpolate
    if opt["interpolate"] is not None:
        kw.update(interpolate=opt["interpolate"], interp_mode='mc' if opt["interp_mode"] is None else opt["interp_mode"])
    elif opt["interp_mode"] is not None:
        raise _Refused("chain: interp_mode= goes with interpolate=")

    def on_clip(plan, clip):
        from . import encoder as _enc
        if not _planar420(clip, (8, 10)):
            raise _Refused(f"chain= takes a planar 4:2:0 source at 8 or 10 bit ({getattr(clip, 'src_format', None)!r})")
        sw, sh, src_depth = int(clip.width), int(clip.height), _sample_depth(clip)
        depth = _enc.bit_depth_of(plan.info)
        matrix = _enc._COLOUR_CODES["matrix"].get(plan.info.color_space, 0)
        sr_matrix = 0
        if sr is not None:
            sr_matrix, sr_full = _sr_source_colour(info, clip, sh)
            kw.update(sr_matrix=sr_matrix, sr_full_range=sr_full)
            matrix = matrix if matrix in (1, 5, 6, 9) else sr_matrix
        try:
            c = _lib.chain(sw, sh, src_depth, **kw)
        except (TypeError, ValueError) as e:
            raise _Refused(f"chain: {e}") from None
        pictures = functools.lru_cache(None)(      # one mihevc_chain_plan_for call per frame count: the clip's for the total, the probe's for the level
            lambda n: _lib.chain_plan(c, target[0], target[1], depth, matrix if sr is not None else 1, sr.scale if sr is not None else 0, int(n or 0)))
        first = pictures(clip.n_frames or total_frames)
        if first is None:
            raise _Refused(f"chain: {c!r} in front of a {target[0]}x{target[1]} session at {depth} bit is not a chain the device takes (no stage on, a size, ratio "
                           "or strength out of range)")
        count = lambda n: int(pictures(n).pictures)
        session_info, rate = _session_info(plan.info, rate=Fraction(first.rate_num, first.rate_den), count=count)
        return replace(plan, info=session_info, rate=rate, count=count, matrix=sr_matrix, send=lambda enc, i, planes: enc.send_chain(*planes, pts=i),
                       setup=((("set_sr_model", (sr,), {}),) if sr is not None else ()) + (("set_chain", (sw, sh, src_depth), dict(chain=c)),))

    return _Plan(info, _session_info(info, size=target)[0], dict(native_formats=True, rgb_formats=False), on_clip=on_clip)


def _plan_options(file_path, info, total_frames, several, row_split, native_rgb, size, deinterlace, tff, denoise, lut, lut_bit_depth, interpolate, interp_mode,
                  upscale, sharpen, antiring, sr_model, sr_target, sr_denoise, chain) -> _Plan:
    """Stage one: the options and the probe alone.  Every refusal that needs no clip is made here; nothing is opened."""
    from . import encoder as _enc
    given = dict(denoise=denoise, upscale=upscale, sr_model=sr_model, interpolate=interpolate, lut=lut, deinterlace=deinterlace, size=size, native_rgb=native_rgb or None,
                 devices=several or None, row_split=row_split or None)
    if chain is not None:
        if any(v is not None for v in given.values()) or tff is not None or sr_target is not None or sr_denoise is not None:
            raise _Refused("chain= takes its filters inside the dict, one device, and none of native_rgb, lut=")
        return _plan_chain(file_path, info, total_frames, chain)
    if isinstance(denoise, int) and not isinstance(denoise, bool) and denoise == 0:
        denoise = None                  # level 0: nothing changes
    given.update(denoise=denoise, row_split=(row_split and several) or None)          # and row_split means nothing on one device
    _refuse_pairs({k for k, v in given.items() if v is not None})
    if sr_model is None and sr_target is not None:
        raise _Refused("sr_target= goes with sr_model=")
    if sr_model is None and sr_denoise is not None:
        raise _Refused("sr_denoise= goes with sr_model=")
    sliced = bool(row_split and several)                    # SlicedEncoder takes planar 4:2:0 only
    flags = dict(native_formats=not sliced, rgb_formats=bool(native_rgb) and not sliced)
    sw0, sh0 = int(info.width), int(info.height)
    plain = lambda **kw: _Plan(info, _session_info(info, **kw)[0], flags)

    if denoise is not None:
        try:
            dn = _lib.denoise_strength(denoise)
        except (TypeError, ValueError):
            raise _Refused(f"denoise={denoise!r} takes a level 0 .. 3 or four thresholds 0 .. 255") from None
        return replace(plain(), on_clip=_needs_plain_frames("denoise=", 2, lambda enc, i, planes: enc.send_denoise(*planes, strength=dn, pts=i)))

    if upscale is not None:
        if isinstance(sharpen, bool) or not isinstance(sharpen, int) or not 0 <= sharpen <= 64 or isinstance(antiring, bool) or not isinstance(antiring, int) or not 0 <= antiring <= 8:
            raise _Refused(f"upscale={upscale!r} takes (w, h), a height or 'auto', sharpen 0 .. 64, antiring 0 .. 8")
        try:
            target = _parse_upscale(upscale, sw0, sh0)
        except (TypeError, ValueError, IndexError):
            raise _Refused(f"upscale={upscale!r} takes (w, h), a height or 'auto'") from None
        if target[0] % 2 or target[1] % 2 or sw0 % 2 or sh0 % 2 or min(sw0, sh0) < 16 or not sw0 <= target[0] <= 4 * sw0 or not sh0 <= target[1] <= 4 * sh0:
            raise _Refused(f"upscale={upscale!r}: {sw0}x{sh0} to {target[0]}x{target[1]} is not an enlargement of even sizes by 1 .. 4 per axis")
        # the road of size=: the session takes the target, the clip is opened at the source's own size
        return replace(plain(size=target), on_clip=_resized("upscale=", "send_upscaled", sharpen=sharpen, antiring=antiring))

    if size is not None:                # rate, level and track follow the coded size
        return replace(plain(size=size), on_clip=_resized("size=", "send_scaled"))

    if sr_model is not None:
        try:
            sr = _load_sr(sr_model, sr_denoise)
        except (OSError, ValueError, TypeError, RuntimeError, KeyError) as e:
            raise _Refused(f"sr_model: {e}") from None
        if min(sw0, sh0) < 4 or (sr.scale == 2 and not hasattr(sr, "convs") and (sw0 % 2 or sh0 % 2)):
            raise _Refused(f"sr_model: a {sw0}x{sh0} source does not fit a scale {sr.scale} model")
        pix = (info.pix_fmt or '').lower()
        yuv = _lib.rgb_format_for(pix) is None          # a Y'CbCr container: read in its own format, converted in front of the network
        if yuv:
            yf = _lib.src_format_for('yuv' + pix[4:] if pix.startswith('yuvj') else pix)
            if yf is None or yf.chroma != 420 or yf.semi_planar or yf.msb_aligned or yf.bit_depth not in (8, 10, 12) or sw0 % 2 or sh0 % 2:
                raise _Refused(f"sr_model= takes an R'G'B' source or a planar 4:2:0 Y'CbCr source at 8, 10 or 12 bit with even sides ({info.pix_fmt!r}, {sw0}x{sh0})")
        try:
            target = sr_target_size(sw0, sh0, sr.scale, sr_target)
        except ValueError as e:
            raise _Refused(str(e)) from None

        def sr_on_clip(plan, clip):
            w, h = int(clip.width), int(clip.height)
            if not yuv:
                fmt = getattr(clip, 'rgb_format', None)
                if fmt is None:
                    raise _Refused(f"sr_model= takes a source that is read as R'G'B' ({getattr(clip, 'src_format', None)!r})")
                sender = "send_sr_fit" if sr_target is not None else "send_sr"
                return replace(plan, send=lambda enc, i, planes: getattr(enc, sender)(fmt, w, h, *planes, pts=i))
            if not _planar420(clip, (8, 10, 12)) or w % 2 or h % 2:
                raise _Refused(f"sr_model= takes a planar 4:2:0 Y'CbCr source at 8, 10 or 12 bit with even sides ({_layout(clip)!r})")
            depth = _sample_depth(clip)
            matrix, full = _sr_source_colour(plan.info, clip, h)
            return replace(plan, matrix=matrix, send=lambda enc, i, planes: enc.send_sr_yuv(w, h, *planes, bit_depth=depth, matrix=matrix, full_range=full, pts=i))

        return replace(plain(size=target), open_flags=dict(native_formats=True, rgb_formats=not yuv), setup=(("set_sr_model", (sr,), {}),), on_clip=sr_on_clip)

    if interpolate is not None:
        if isinstance(interpolate, bool) or not isinstance(interpolate, int) or interpolate not in (2, 3, 4) or interp_mode not in _lib.INTERP_MODES:
            raise _Refused(f"interpolate={interpolate!r} takes 2, 3 or 4, interp_mode 'mc' or 'blend'")
        count = lambda n: (n - 1) * interpolate + 1
        send = lambda enc, i, planes: enc.send_interpolate(*planes, factor=interpolate, mode=interp_mode, pts=i * interpolate)
        # the session, its level and the track run at the multiplied rate
        return replace(plain(rate=interpolate, count=count), count=count, on_clip=_needs_plain_frames("interpolate=", 2, send))

    if lut is not None:
        from . import lut3d
        if lut_bit_depth not in (8, 10):
            raise _Refused("lut= takes a .cube path, an (n, n, n, 3) table or 'hdr-to-sdr', lut_bit_depth 8 or 10")
        try:
            if isinstance(lut, str) and lut == 'hdr-to-sdr':
                from .utils import parse_master_display
                transfer = 'hlg' if (info.color_transfer or '').lower() == 'arib-std-b67' else 'pq'
                peak = parse_master_display(info.master_display).lum[0] / 10000.0 if (info.master_display or '').strip() else 1000.0
                table = lut3d.hdr_to_sdr(65, transfer, min(max(peak, lut3d.SDR_PEAK_NITS), 10000.0))
            elif isinstance(lut, (str, Path)):
                table = lut3d.quantise(lut3d.read_cube(lut))
            else:
                table = lut3d.as_uint16(lut)
        except (OSError, TypeError, ValueError) as e:
            raise _Refused(f"lut={lut if isinstance(lut, (str, Path)) else type(lut).__name__!r}: {e}") from None
        src_matrix = _enc._COLOUR_CODES["matrix"].get(info.color_space, 9 if info.hdr else 1)
        src_full = (info.pix_fmt or '').lower().startswith('yuvj')

        def lut_on_clip(plan, clip):
            w, h = int(plan.info.width), int(plan.info.height)
            if not _planar420(clip, (8, 10, 12)) or w % 2 or h % 2 or min(w, h) < 16:
                raise _Refused(f"lut= takes a planar 4:2:0 source at 8, 10 or 12 bit, width and height even ({_layout(clip)!r}, {w}x{h})")
            depth = _sample_depth(clip)
            return replace(plan, send=lambda enc, i, planes: enc.send_lut3d(*planes, bit_depth=depth, matrix=src_matrix, full_range=src_full, pts=i))

        # the session, its level and the track are those of an SDR clip
        return replace(plain(sdr_depth=lut_bit_depth), own_depth=True, setup=(("set_lut3d", (table,), {}),), on_clip=lut_on_clip)

    if deinterlace is not None:
        if deinterlace not in ('frame', 'field', 'auto', 'ivtc', 'match'):
            raise _Refused(f"deinterlace={deinterlace!r} takes 'frame', 'field', 'auto', 'ivtc' or 'match'")
        order = _field_order(file_path, tff, deinterlace)
        if deinterlace in ('ivtc', 'match'):
            decimate = deinterlace == 'ivtc'            # 'ivtc': the session runs at 4/5 of the source's rate, as a fraction
            send = lambda enc, i, planes: enc.send_fieldmatch(*planes, tff=bool(order), decimate=decimate, deint=True, pts=i)
            count = (lambda n: n * 4 // 5) if decimate else int
            session_info, rate = _session_info(info, rate=Fraction(4, 5), count=count) if decimate else _session_info(info)
            return _Plan(info, session_info, flags, rate=rate, count=count, on_clip=_needs_plain_frames("deinterlace=", 4, send))
        if order is not None:
            field_rate = deinterlace == 'field'
            step = 2 if field_rate else 1
            send = lambda enc, i, planes: enc.send_deint(*planes, tff=bool(order), field_rate=field_rate, pts=i * step)
            count = lambda n: n * step
            session_info = _session_info(info, rate=2, count=count)[0] if field_rate else _session_info(info)[0]
            return _Plan(info, session_info, flags, count=count, on_clip=_needs_plain_frames("deinterlace=", 4, send))
    return plain()


def _plan_clip(plan: _Plan, clip, several: bool, sliced: bool) -> _Plan:
    """Stage two: what only the opened clip can say.  The depth in the file's own header outranks the probe (a y4m tagged C420p10 probed as SDR); the option's
    own checks and its sender; without an option, the sender that takes the clip's layout."""
    from . import encoder as _enc
    if not plan.own_depth and clip.bit_depth > 8 and _enc.bit_depth_of(plan.info) == 8:
        fixed = copy.copy(plan.info)
        fixed.pix_fmt = 'yuv420p10le'
        plan = replace(plan, info=fixed)
    if plan.on_clip is not None:
        return plan.on_clip(plan, clip)
    fmt = _layout(clip)     # not the session's own layout: converted on the device (send_fmt), an RGB source matrixed and decimated there (send_rgb)
    if fmt is not None and sliced:
        raise _Refused(f"a {fmt!r} source cannot be split by rows")
    if several:             # three planes each, the layout after them where it is not the session's own
        return replace(plan, send=lambda sh, i, planes: sh.send(*(tuple(planes) + (None, None))[:3], *(() if fmt is None else (fmt,))))
    if fmt is None:
        return replace(plan, send=lambda enc, i, planes: enc.send(*planes, pts=i))
    sender = "send_rgb" if getattr(clip, 'rgb_format', None) is not None else "send_fmt"
    return replace(plan, send=lambda enc, i, planes: getattr(enc, sender)(fmt, *planes, pts=i))


def encode_file(file_path: Path, out_path: Path, info: VideoInfo, progress_callback: Optional[Callable[[str, int, int], None]] = None,
                total_frames: int = 1, stop_event: Optional[threading.Event] = None, device: Optional[int] = None, debug: bool = False,
                devices=None, row_split: bool = False, native_rgb: bool = False, size=None, deinterlace: Optional[str] = None,
                tff: Optional[bool] = None, denoise=None, lut=None, lut_bit_depth: int = 8, interpolate: Optional[int] = None, interp_mode: str = 'mc',
                upscale=None, sharpen: int = 8, antiring: int = 8, sr_model=None, sr_target=None, sr_denoise=None, chain: Optional[dict] = None) -> int:
    """Encode `file_path` to `out_path` (MP4/hvc1) on an MI355X.  Returns 0 on success, 1 on failure/cancel —
    the same (returncode) shape `run_ffmpeg` gives `convert_video` (core/transcoder.py:497-535).
    devices: several of them take one clip: GOP chunks round-robin (ShardedEncoder) or, with row_split, every picture split by CTU rows (SlicedEncoder).
    native_rgb: a container probed as one of the RGB pixel formats of _lib.rgb_format_for is decoded to that format and converted on the device
    (Encoder.send_rgb) instead of by swscale; the session signals the probed matrix, BT.709 when that is `gbr` or unknown.
    size=(w, h): the session, its level and the MP4 track take this size and every picture of the source, delivered at its own size, is scaled down on the device
    (Encoder.send_scaled): planar 4:2:0 sources, per axis at most 4:1.
    deinterlace: the source's frames are woven interlaced frames, deinterlaced on the device (Encoder.send_deint).  'frame': one picture per
    frame; 'field': one per field, so the session, its level, the rate figures and the MP4 track run at twice the frame rate; 'auto': 'frame' when the source
    says it is interlaced (the y4m header's It / Ib tag, else ffprobe's field_order), nothing otherwise.  tff: the field order, None to take the source's word
    (top field first when it has none).  Planar 4:2:0 sources at the session's depth.  'ivtc' and 'match': the frames carry film in fields (3:2 pulldown) and go
    through inverse telecine instead (Encoder.send_fieldmatch), with the same field-order lookup: 'ivtc' matches fields and drops one frame of
    every five, so the session, its level, the progress total and the MP4 track run at exactly 4/5 of the source rate (30000/1001 gives 24000/1001); 'match'
    only matches fields and keeps the rate.  'auto' keeps meaning the deinterlacer.
    denoise: a level 1 .. 3 or a tuple of four thresholds (Encoder.send_denoise): every frame is denoised on the device in front of the session.
    None and 0: nothing changes.  Planar 4:2:0 sources at the session's depth.
    lut: every frame goes through a 3D colour table on the device (Encoder.send_lut3d): the path of a .cube file, an (n, n, n, 3) array, or
    'hdr-to-sdr' for the built-in table of lut3d.hdr_to_sdr (the transfer from the probe, PQ unless it says HLG; peak_nits from the probed master_display when
    there is one).  The session opens as SDR whatever the probe says of the source: 8 bit (lut_bit_depth=10: Main10), colour description 1/1/1, no HDR10 SEI, the
    level and tier of an SDR clip; the reader keeps delivering the source's own planar 4:2:0 frames at 8, 10 or 12 bit, and the source's matrix is the probed one
    (BT.2020 for HDR, else BT.709 when unknown).
    interpolate: 2, 3 or 4: the frame rate is multiplied on the device (Encoder.send_interpolate), interp_mode 'mc' by motion-compensated
    interpolation, 'blend' by blending; the session, its level, the rate figures and the MP4 track run at that multiple of the probed rate, n frames give
    interpolate * (n - 1) + 1 pictures, and the progress total counts pictures.  None: nothing changes.  Planar 4:2:0 sources at the session's depth.
    upscale: (w, h), a target height, or 'auto' for upscale_target's rule: the session, its level and the MP4 track take that size and every picture of the
    source, delivered at its own size, is enlarged on the device (Encoder.send_upscaled) with sharpen (0 .. 64 sixteenths) and antiring (0 .. 8
    eighths).  None: nothing changes.  Planar 4:2:0 sources, per axis between 1:1 and 1:4.
    sr_model: the path of an RRDBNet or SRVGGNetCompact .pth file, a state dict, or an hevc_amd.sr.RrdbNet / CompactNet (hevc_amd.sr.load_model chooses by
    the keys): every picture is enlarged by the network on the device.  A pair (model, denoise partner) of compact models with
    sr_denoise = 0 .. 1 is the compact family's denoise strength (realesr-general-x4v3 with realesr-general-wdn-x4v3): the two are blended on the host
    (hevc_amd.sr.blend), sr_denoise being the weight of the FIRST model.  The reference's tool has a noise level 0 .. 3 and states no mapping of it onto this
    strength, so none is made up here: the caller gives the strength.  sr_denoise with a single model or an RRDBNet, or a pair without it, is an error.  A
    compact model of scale 2 takes odd R'G'B' source sides.  A container that probes as one of the RGB pixel formats is asked for as it is, as native_rgb=True asks (Encoder.send_sr).  A planar 4:2:0
    Y'CbCr container at 8, 10 or 12 bit is read in its own format and brought to R'G'B' on the device (Encoder.send_sr_yuv): its matrix is the probed one, and
    when the probe does not know it BT.601 below 720 lines and BT.709 from there on, which is what players and swscale assume; its range is the probed one
    (yuvj* files read directly are full range; the pipe hands yuvj* over as limited range).  Any other format (4:2:2, 4:4:4, semi-planar) is refused by name.
    sr_target: None: the session, its level and the MP4 track open at scale x the source size.  'auto', a height or (w, h) (sr_target_size): they open at that
    size and the network's picture is scaled down to it on the device; 'auto' is what the reference's restoration tool does.  sr_target without sr_model is
    refused.  There is no tiling: a frame the device cannot hold ends the run.
    What goes together (_TOGETHER, judged in one place before anything is opened): size=, deinterlace=, denoise=, lut=, interpolate=, upscale= and sr_model= are
    the source filters; outside chain= a run takes one of them at the most, on one device: none of them goes with several devices or sliced sessions.
    native_rgb stands beside size= (where an RGB clip is then refused), beside sr_model= (which reads an RGB container as it is anyway) and beside several
    devices, and beside no other filter.
    chain: a dict of the options above that go TOGETHER (Encoder.set_chain / send_chain): deinterlace= and tff=, denoise=, one of size= | upscale=
    (sharpen=, antiring=) | sr_model= (sr_target=, sr_denoise=), interpolate= and interp_mode=, each meaning what the option of that name means; the filters run
    in that fixed order on the device, field and denoise at the source's size, interpolation at the session's.  The session's size, level, rate figures, the
    progress total and the MP4 track follow the chain's size and rate (hevc_amd/csrc/chain_plan.h); 'ivtc' sets the rate as an exact fraction.  Planar 4:2:0
    sources at 8 or 10 bit on one device; chain= together with any of those options outside the dict, with native_rgb, lut= or several devices is refused.
    chain=dict(denoise=n, sr_model=p, sr_target='auto', interpolate=k) is the whole process_video of the reference's restoration tool on the device."""
    from . import encoder as _enc, mp4, yuvio
    from .transcoder import calculate_apple_hevc_level, calculate_dynamic_values
    name = Path(file_path).name
    several = bool(devices and len(devices) > 1)            # one clip over several GPUs: GOP chunks round-robin, or every picture split by CTU rows
    clip = mux = None
    ok = False
    try:
        plan = _plan_options(file_path, info, total_frames, several, row_split, native_rgb, size, deinterlace, tff, denoise, lut, lut_bit_depth, interpolate,
                             interp_mode, upscale, sharpen, antiring, sr_model, sr_target, sr_denoise, chain)
        clip = yuvio.open_any(Path(file_path), plan.clip_info, **plan.open_flags)
        plan = _plan_clip(plan, clip, several, bool(row_split and several))
        crf, _cq, maxrate, bufsize, gop = calculate_dynamic_values(plan.info)
        level, tier = calculate_apple_hevc_level(plan.info)
        cfg = _enc.config_for(plan.info, crf, maxrate, bufsize, gop, level, tier)
        if plan.rate is not None:
            cfg.fps_num, cfg.fps_den = plan.rate.numerator, plan.rate.denominator
        matrix = 1 if getattr(clip, 'rgb_format', None) is not None else plan.matrix
        if matrix and cfg.matrix not in (1, 5, 6, 9):
            cfg.matrix = matrix
        total = plan.count(clip.n_frames or total_frames)
        wants_audio = bool(info.audio_channels and info.audio_channels > 0) and Path(file_path).suffix.lower() not in ('.y4m', '.yuv')
        video_path = Path(out_path).with_suffix('.video.mp4') if wants_audio else Path(out_path)
        mux = mp4.Mp4Writer(video_path, cfg)
        n_out = 0

        def drain(packets):             # (data, pts, key, dts) of a session, (data, pts, key) of several
            nonlocal n_out
            for packet in packets:
                mux.add_sample(*packet)
                n_out += 1
            if progress_callback:
                try:
                    progress_callback(name, n_out, total)
                except Exception:
                    logger.debug("progress_callback raised", exc_info=True)

        if several:
            enc = (_enc.SlicedEncoder if row_split else _enc.ShardedEncoder)(cfg, devices)
            session, ready, finish = contextlib.closing(enc), enc.ready, enc.finish      # close() joins the workers (abort) before any session is closed
        else:
            enc = session = _enc.Encoder(cfg, device=device or 0)
            ready = enc.packets_dts

            def finish():
                enc.flush()
                return enc.packets_dts()

        with session:
            for method, args, kw in plan.setup:
                getattr(enc, method)(*args, **kw)
            for i, planes in enumerate(clip.frames()):
                if stop_event is not None and stop_event.is_set():
                    return 1
                plan.send(enc, i, planes)
                drain(ready())
            drain(finish())
            headers = enc.headers()
        if n_out == 0:
            return 1
        mux.finish(headers)
        mux = None
        if not _carry_audio(wants_audio, video_path, file_path, out_path, plan.info):
            return 1
        ok = True
        return 0
    except _Refused as e:
        logger.error("%s: %s", name, e)
        return 1
    finally:
        if mux is not None and not ok:
            mux.abort()                             # cancel, failure or exception: no .mdat.tmp and no open handle stay behind
        if clip is not None:
            clip.close()
