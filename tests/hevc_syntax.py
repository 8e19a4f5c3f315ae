"""An independent reader of the H.265 syntax this project's encoder emits -- TEST INFRASTRUCTURE, NOT PRODUCT.

Written clause by clause from ITU-T H.265 (v1, 04/2013, and the clause numbers it keeps in later editions), not from this repository's
writer (hevc_amd/csrc/bitstream.cpp) or decoder (oracle/hevc_dec.c): it imports neither package and reads none of their files, and its
tables are its own transcription of the standard.  tests/test_syntax_independent.py checks that this module imports only the standard
library and numpy.

It parses the subset the encoder emits: Main and Main 10, 4:2:0, CTB 32, minimum CB 8, TU 4..32, tiles, several slices per picture, SAO,
intra NxN, 2Nx2N inter, P and B slices with one picture per list, sign data hiding, and the SEI messages buffering period, picture timing,
mastering display colour volume, content light level and (in suffix SEI NAL units) decoded picture hash.  Anything outside that subset --
including any tool flag the encoder never sets (TMVP, transform skip, cu_qp_delta, AMP, PCM, WPP, dependent slices, weighted prediction,
scaling lists, long-term pictures, list modification, more than one reference per list) being 1 -- raises Unsupported instead of being guessed.

parse_stream(bytes) -> Stream with the parameter sets, the SEI and AUD payloads and one Picture per coded picture in decoding order: NAL type,
POC, slice types and QPs, a per-8x8 record of every coding-unit decision, the coefficient levels in picture raster, the SAO parameters per CTB,
the decoded picture hash that follows it and the number of times each (syntax element, ctxInc, initType) was decoded.  tests/hevc_recon.py
reconstructs the samples from it.
"""
from __future__ import annotations

import collections

import numpy as np


class Unsupported(Exception):
    """syntax outside the subset this reader implements"""


class ParseError(Exception):
    """the stream breaks a rule of H.265 that this reader checks"""


def need(cond, msg):
    if not cond:
        raise ParseError(msg)


def subset(cond, msg):
    if not cond:
        raise Unsupported(msg)


# ================================================================ B.2 byte stream, 7.3.1 NAL units
def split_annexb(stream: bytes) -> list:
    """B.2: NAL units between start code prefixes 0x000001.  A NAL unit never ends in 0x00 (7.4.2), so trailing zero bytes belong to the next
    start code (zero_byte) or are trailing_zero_8bits."""
    out, n = [], len(stream)
    start = stream.find(b"\x00\x00\x01", 0)
    need(start >= 0, "no start code")
    need(all(b == 0 for b in stream[:start]), "leading bytes before the first start code are not zero")
    while start >= 0:
        i = start + 3
        nxt = stream.find(b"\x00\x00\x01", i)
        end = n if nxt < 0 else nxt
        nal = stream[i:end].rstrip(b"\x00")
        need(len(nal) >= 2, "empty NAL unit")
        out.append(nal)
        start = nxt
    return out


def nal_to_rbsp(nal: bytes):
    """7.3.1.1 / 7.4.2: drop each emulation_prevention_three_byte (0x03 after 0x0000).  Returns (rbsp, nal_pos) where nal_pos[k] is the index in
    the NAL unit of RBSP byte k (and nal_pos[len(rbsp)] = len(nal)); entry points count NAL bytes (7.4.7.1)."""
    rbsp, pos, zeros = bytearray(), [], 0
    for i, b in enumerate(nal):
        if zeros >= 2 and b == 3:
            need(i + 1 == len(nal) or nal[i + 1] <= 3, "0x000003 followed by a byte above 3")
            zeros = 0
            continue
        need(not (zeros >= 2 and b <= 2), "start code emulation inside a NAL unit")
        rbsp.append(b)
        pos.append(i)
        zeros = zeros + 1 if b == 0 else 0
    pos.append(len(nal))
    return bytes(rbsp), pos


class Bits:
    """7.2 / 9.2: u(n), ue(v), se(v), more_rbsp_data(), trailing bits"""

    def __init__(self, data: bytes, pos: int = 0):
        self.data, self.pos, self.end = data, pos, 8 * len(data)

    def u1(self):
        need(self.pos < self.end, "read past the end of the RBSP")
        b = (self.data[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return b

    def u(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.u1()
        return v

    def ue(self):                                   # 9.2 Exp-Golomb
        lz = 0
        while self.u1() == 0:
            lz += 1
            need(lz < 32, "ue(v) longer than 32 bits")
        return (1 << lz) - 1 + self.u(lz)

    def se(self):                                   # 9.2.2 Table 9-3
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)

    def byte_aligned(self):
        return self.pos & 7 == 0

    def more_rbsp_data(self):                       # 7.2: anything before the last 1 bit of the RBSP
        last = len(self.data) - 1
        while last >= 0 and self.data[last] == 0:
            last -= 1
        need(last >= 0, "RBSP without rbsp_stop_one_bit")
        b = self.data[last]
        stop = 8 * last + 7 - ((b & -b).bit_length() - 1)
        return self.pos < stop

    def rbsp_trailing_bits(self):                   # 7.3.2.11
        need(self.u1() == 1, "rbsp_stop_one_bit is not 1")
        while not self.byte_aligned():
            need(self.u1() == 0, "rbsp_alignment_zero_bit is not 0")
        need(self.pos == self.end, "bytes after rbsp_trailing_bits")

    def byte_alignment(self):                       # 7.3.2.12
        need(self.u1() == 1, "alignment_bit_equal_to_one is not 1")
        while not self.byte_aligned():
            need(self.u1() == 0, "alignment_bit_equal_to_zero is not 0")


# ================================================================ 7.3.3 profile_tier_level, E.2.2 hrd_parameters
def profile_tier_level(r: Bits, max_sub_layers_minus1):
    p = {"profile_space": r.u(2), "tier_flag": r.u1(), "profile_idc": r.u(5), "compat": r.u(32),
         "progressive_source_flag": r.u1(), "interlaced_source_flag": r.u1(), "non_packed_constraint_flag": r.u1(),
         "frame_only_constraint_flag": r.u1()}
    r.u(32)
    r.u(11)
    r.u1()                                          # general_inbld_flag / reserved
    p["level_idc"] = r.u(8)
    present = [(r.u1(), r.u1()) for _ in range(max_sub_layers_minus1)]
    if max_sub_layers_minus1 > 0:
        for _ in range(max_sub_layers_minus1, 8):
            r.u(2)
    for prof, lev in present:
        if prof:
            r.u(32), r.u(32), r.u(24)
        if lev:
            r.u(8)
    return p


def sub_layer_hrd_parameters(r: Bits, cpb_cnt, sub_pic):
    out = []
    for _ in range(cpb_cnt):
        e = {"bit_rate_value_minus1": r.ue(), "cpb_size_value_minus1": r.ue()}
        if sub_pic:
            e["cpb_size_du_value_minus1"], e["bit_rate_du_value_minus1"] = r.ue(), r.ue()
        e["cbr_flag"] = r.u1()
        out.append(e)
    return out


def hrd_parameters(r: Bits, common, max_sub_layers_minus1):
    h = {"nal": 0, "vcl": 0, "sub_pic_hrd_params_present_flag": 0, "initial_cpb_removal_delay_length_minus1": 23,
         "au_cpb_removal_delay_length_minus1": 23, "dpb_output_delay_length_minus1": 23}
    if common:
        h["nal"], h["vcl"] = r.u1(), r.u1()
        if h["nal"] or h["vcl"]:
            h["sub_pic_hrd_params_present_flag"] = r.u1()
            if h["sub_pic_hrd_params_present_flag"]:
                r.u(8), r.u(5), r.u1(), r.u(5)
            h["bit_rate_scale"], h["cpb_size_scale"] = r.u(4), r.u(4)
            if h["sub_pic_hrd_params_present_flag"]:
                r.u(4)
            h["initial_cpb_removal_delay_length_minus1"] = r.u(5)
            h["au_cpb_removal_delay_length_minus1"] = r.u(5)
            h["dpb_output_delay_length_minus1"] = r.u(5)
    h["sub_layers"] = []
    for _ in range(max_sub_layers_minus1 + 1):
        s = {"fixed_pic_rate_general_flag": r.u1()}
        s["fixed_pic_rate_within_cvs_flag"] = 1 if s["fixed_pic_rate_general_flag"] else r.u1()
        s["low_delay_hrd_flag"] = 0
        if s["fixed_pic_rate_within_cvs_flag"]:
            s["elemental_duration_in_tc_minus1"] = r.ue()
        else:
            s["low_delay_hrd_flag"] = r.u1()
        s["cpb_cnt_minus1"] = 0 if s["low_delay_hrd_flag"] else r.ue()
        if h["nal"]:
            s["nal"] = sub_layer_hrd_parameters(r, s["cpb_cnt_minus1"] + 1, h["sub_pic_hrd_params_present_flag"])
        if h["vcl"]:
            s["vcl"] = sub_layer_hrd_parameters(r, s["cpb_cnt_minus1"] + 1, h["sub_pic_hrd_params_present_flag"])
        h["sub_layers"].append(s)
    return h


# ================================================================ 7.3.2.1 VPS
def parse_vps(r: Bits):
    v = {"id": r.u(4), "base_layer_internal_flag": r.u1(), "base_layer_available_flag": r.u1(), "max_layers_minus1": r.u(6),
         "max_sub_layers_minus1": r.u(3), "temporal_id_nesting_flag": r.u1()}
    need(r.u(16) == 0xFFFF, "vps_reserved_0xffff_16bits")
    v["ptl"] = profile_tier_level(r, v["max_sub_layers_minus1"])
    v["sub_layer_ordering_info_present_flag"] = r.u1()
    v["ordering"] = []
    for _ in range(0 if v["sub_layer_ordering_info_present_flag"] else v["max_sub_layers_minus1"], v["max_sub_layers_minus1"] + 1):
        v["ordering"].append((r.ue(), r.ue(), r.ue()))
    v["max_layer_id"] = r.u(6)
    v["num_layer_sets_minus1"] = r.ue()
    for _ in range(v["num_layer_sets_minus1"]):
        r.u(v["max_layer_id"] + 1)
    v["timing_info_present_flag"] = r.u1()
    if v["timing_info_present_flag"]:
        v["num_units_in_tick"], v["time_scale"] = r.u(32), r.u(32)
        if r.u1():
            r.ue()
        v["num_hrd_parameters"] = r.ue()
        for i in range(v["num_hrd_parameters"]):
            r.ue()
            cprms = r.u1() if i > 0 else 1
            hrd_parameters(r, cprms, v["max_sub_layers_minus1"])
    subset(r.u1() == 0, "vps_extension_flag")
    r.rbsp_trailing_bits()
    return v


# ================================================================ 7.3.7 st_ref_pic_set, 7.4.8
def st_ref_pic_set(r: Bits, idx, num_sets, sets):
    inter = r.u1() if idx != 0 else 0
    if inter:
        delta_idx_minus1 = r.ue() if idx == num_sets else 0
        sign, abs_minus1 = r.u1(), r.ue()
        ref = sets[idx - (delta_idx_minus1 + 1)]
        delta_rps = (1 - 2 * sign) * (abs_minus1 + 1)
        nd = len(ref["s0"]) + len(ref["s1"])
        used, use_delta = [], []
        for _ in range(nd + 1):
            u = r.u1()
            used.append(u)
            use_delta.append(1 if u else r.u1())
        n0 = len(ref["s0"])
        s0, s1 = [], []                             # (7-61) and (7-62)
        for j in range(len(ref["s1"]) - 1, -1, -1):
            d = ref["s1"][j][0] + delta_rps
            if d < 0 and use_delta[n0 + j]:
                s0.append((d, used[n0 + j]))
        if delta_rps < 0 and use_delta[nd]:
            s0.append((delta_rps, used[nd]))
        for j in range(n0):
            d = ref["s0"][j][0] + delta_rps
            if d < 0 and use_delta[j]:
                s0.append((d, used[j]))
        for j in range(n0 - 1, -1, -1):
            d = ref["s0"][j][0] + delta_rps
            if d > 0 and use_delta[j]:
                s1.append((d, used[j]))
        if delta_rps > 0 and use_delta[nd]:
            s1.append((delta_rps, used[nd]))
        for j in range(len(ref["s1"])):
            d = ref["s1"][j][0] + delta_rps
            if d > 0 and use_delta[n0 + j]:
                s1.append((d, used[n0 + j]))
        return {"s0": s0, "s1": s1, "inter": 1}
    nneg, npos = r.ue(), r.ue()
    s0, s1, d = [], [], 0
    for _ in range(nneg):
        d -= r.ue() + 1
        s0.append((d, r.u1()))
    d = 0
    for _ in range(npos):
        d += r.ue() + 1
        s1.append((d, r.u1()))
    return {"s0": s0, "s1": s1, "inter": 0}


# ================================================================ 7.3.2.2 SPS, E.2.1 VUI
def vui_parameters(r: Bits, max_sub_layers_minus1):
    v = {"aspect_ratio_info_present_flag": r.u1()}
    if v["aspect_ratio_info_present_flag"]:
        v["aspect_ratio_idc"] = r.u(8)
        if v["aspect_ratio_idc"] == 255:
            v["sar_width"], v["sar_height"] = r.u(16), r.u(16)
    if r.u1():
        v["overscan_appropriate_flag"] = r.u1()
    v["video_signal_type_present_flag"] = r.u1()
    v["colour_primaries"] = v["transfer_characteristics"] = v["matrix_coeffs"] = 2
    v["video_full_range_flag"] = 0
    if v["video_signal_type_present_flag"]:
        v["video_format"], v["video_full_range_flag"] = r.u(3), r.u1()
        if r.u1():
            v["colour_primaries"], v["transfer_characteristics"], v["matrix_coeffs"] = r.u(8), r.u(8), r.u(8)
    v["chroma_loc_info_present_flag"] = r.u1()
    if v["chroma_loc_info_present_flag"]:
        v["chroma_sample_loc_type_top_field"], v["chroma_sample_loc_type_bottom_field"] = r.ue(), r.ue()
    v["neutral_chroma_indication_flag"], v["field_seq_flag"], v["frame_field_info_present_flag"] = r.u1(), r.u1(), r.u1()
    if r.u1():
        v["default_display_window"] = (r.ue(), r.ue(), r.ue(), r.ue())
    v["timing_info_present_flag"] = r.u1()
    v["hrd"] = None
    if v["timing_info_present_flag"]:
        v["num_units_in_tick"], v["time_scale"] = r.u(32), r.u(32)
        if r.u1():
            v["num_ticks_poc_diff_one_minus1"] = r.ue()
        if r.u1():
            v["hrd"] = hrd_parameters(r, 1, max_sub_layers_minus1)
    if r.u1():
        v["bitstream_restriction"] = (r.u1(), r.u1(), r.u1(), r.ue(), r.ue(), r.ue(), r.ue(), r.ue())
    return v


def parse_sps(r: Bits):
    s = {"vps_id": r.u(4), "max_sub_layers_minus1": r.u(3), "temporal_id_nesting_flag": r.u1()}
    s["ptl"] = profile_tier_level(r, s["max_sub_layers_minus1"])
    s["id"] = r.ue()
    s["chroma_format_idc"] = r.ue()
    subset(s["chroma_format_idc"] == 1, "chroma_format_idc other than 4:2:0")
    s["width"], s["height"] = r.ue(), r.ue()
    s["conf_win"] = (r.ue(), r.ue(), r.ue(), r.ue()) if r.u1() else (0, 0, 0, 0)
    s["bit_depth_luma"], s["bit_depth_chroma"] = r.ue() + 8, r.ue() + 8
    subset(s["bit_depth_luma"] in (8, 10) and s["bit_depth_chroma"] == s["bit_depth_luma"], "bit depth other than Main / Main 10")
    s["log2_max_poc_lsb"] = r.ue() + 4
    s["sub_layer_ordering_info_present_flag"] = r.u1()
    s["ordering"] = []
    for _ in range(0 if s["sub_layer_ordering_info_present_flag"] else s["max_sub_layers_minus1"], s["max_sub_layers_minus1"] + 1):
        s["ordering"].append({"max_dec_pic_buffering_minus1": r.ue(), "max_num_reorder_pics": r.ue(), "max_latency_increase_plus1": r.ue()})
    s["min_cb_log2"] = r.ue() + 3
    s["ctb_log2"] = s["min_cb_log2"] + r.ue()
    s["min_tb_log2"] = r.ue() + 2
    s["max_tb_log2"] = s["min_tb_log2"] + r.ue()
    s["max_transform_hierarchy_depth_inter"], s["max_transform_hierarchy_depth_intra"] = r.ue(), r.ue()
    subset((s["ctb_log2"], s["min_cb_log2"], s["min_tb_log2"]) == (5, 3, 2) and s["max_tb_log2"] == 5, "block sizes other than CTB 32 / CB 8 / TB 4..32")
    subset(r.u1() == 0, "scaling_list_enabled_flag")
    s["amp_enabled_flag"] = r.u1()
    subset(s["amp_enabled_flag"] == 0, "amp_enabled_flag")
    s["sao_enabled_flag"] = r.u1()
    subset(r.u1() == 0, "pcm_enabled_flag")
    n = r.ue()
    need(n <= 64, "num_short_term_ref_pic_sets > 64")
    s["st_rps"] = []
    for i in range(n):
        s["st_rps"].append(st_ref_pic_set(r, i, n, s["st_rps"]))
    subset(r.u1() == 0, "long_term_ref_pics_present_flag")
    s["temporal_mvp_enabled_flag"] = r.u1()
    subset(s["temporal_mvp_enabled_flag"] == 0, "sps_temporal_mvp_enabled_flag")
    s["strong_intra_smoothing_enabled_flag"] = r.u1()
    s["vui"] = vui_parameters(r, s["max_sub_layers_minus1"]) if r.u1() else None
    subset(r.u1() == 0, "sps_extension_present_flag")
    r.rbsp_trailing_bits()
    need(s["width"] % (1 << s["min_cb_log2"]) == 0 and s["height"] % (1 << s["min_cb_log2"]) == 0, "picture size not a multiple of MinCbSizeY")
    return s


# ================================================================ 7.3.2.3 PPS
def parse_pps(r: Bits):
    p = {"id": r.ue(), "sps_id": r.ue()}
    subset(r.u1() == 0, "dependent_slice_segments_enabled_flag")
    subset(r.u1() == 0, "output_flag_present_flag")
    p["num_extra_slice_header_bits"] = r.u(3)
    p["sign_data_hiding_enabled_flag"] = r.u1()
    p["cabac_init_present_flag"] = r.u1()
    p["num_ref_idx_default"] = (r.ue() + 1, r.ue() + 1)
    p["init_qp"] = 26 + r.se()
    subset(r.u1() == 0, "constrained_intra_pred_flag")
    subset(r.u1() == 0, "transform_skip_enabled_flag")
    subset(r.u1() == 0, "cu_qp_delta_enabled_flag")
    p["cb_qp_offset"], p["cr_qp_offset"] = r.se(), r.se()
    p["slice_chroma_qp_offsets_present_flag"] = r.u1()
    subset(r.u1() == 0, "weighted_pred_flag")
    subset(r.u1() == 0, "weighted_bipred_flag")
    subset(r.u1() == 0, "transquant_bypass_enabled_flag")
    p["tiles_enabled_flag"] = r.u1()
    subset(r.u1() == 0, "entropy_coding_sync_enabled_flag")
    p["tile_cols"], p["tile_rows"], p["uniform_spacing_flag"] = 1, 1, 1
    p["col_widths"] = p["row_heights"] = None
    if p["tiles_enabled_flag"]:
        p["tile_cols"], p["tile_rows"] = r.ue() + 1, r.ue() + 1
        p["uniform_spacing_flag"] = r.u1()
        if not p["uniform_spacing_flag"]:
            p["col_widths"] = [r.ue() + 1 for _ in range(p["tile_cols"] - 1)]
            p["row_heights"] = [r.ue() + 1 for _ in range(p["tile_rows"] - 1)]
        p["loop_filter_across_tiles_enabled_flag"] = r.u1()
    p["loop_filter_across_slices_enabled_flag"] = r.u1()
    p["deblocking_filter_override_enabled_flag"] = p["pps_deblocking_filter_disabled_flag"] = 0
    if r.u1():
        p["deblocking_filter_override_enabled_flag"] = r.u1()
        p["pps_deblocking_filter_disabled_flag"] = r.u1()
        if not p["pps_deblocking_filter_disabled_flag"]:
            p["beta_offset_div2"], p["tc_offset_div2"] = r.se(), r.se()
    subset(r.u1() == 0, "pps_scaling_list_data_present_flag")
    subset(r.u1() == 0, "lists_modification_present_flag")
    p["log2_parallel_merge_level"] = r.ue() + 2
    subset(r.u1() == 0, "slice_segment_header_extension_present_flag")
    subset(r.u1() == 0, "pps_extension_present_flag")
    r.rbsp_trailing_bits()
    return p


# ================================================================ 7.3.5 SEI (D.2.2, D.2.3, D.2.28, D.2.35)
def parse_sei(r: Bits, sps, nal_type):
    msgs = []
    while True:
        ptype = 0
        while True:
            b = r.u(8)
            ptype += b
            if b != 255:
                break
        size = 0
        while True:
            b = r.u(8)
            size += b
            if b != 255:
                break
        start = r.pos
        m = {"type": ptype, "size": size}
        hrd = sps["vui"]["hrd"] if sps and sps["vui"] else None
        if ptype == 0:                                          # D.2.2 buffering_period
            subset(hrd is not None, "buffering period without HRD parameters")
            m["sps_id"] = r.ue()
            irap = 0
            if not hrd["sub_pic_hrd_params_present_flag"]:
                irap = r.u1()
            if irap:
                r.u(hrd["au_cpb_removal_delay_length_minus1"] + 1), r.u(hrd["dpb_output_delay_length_minus1"] + 1)
            m["concatenation_flag"] = r.u1()
            m["au_cpb_removal_delay_delta_minus1"] = r.u(hrd["au_cpb_removal_delay_length_minus1"] + 1)
            n = hrd["initial_cpb_removal_delay_length_minus1"] + 1
            for which in ("nal", "vcl"):
                if hrd[which]:
                    m[which] = []
                    for _ in range(hrd["sub_layers"][0]["cpb_cnt_minus1"] + 1):
                        e = (r.u(n), r.u(n))
                        if hrd["sub_pic_hrd_params_present_flag"] or irap:
                            e += (r.u(n), r.u(n))
                        m[which].append(e)
        elif ptype == 1:                                        # D.2.3 pic_timing
            if sps["vui"]["frame_field_info_present_flag"]:
                m["pic_struct"], m["source_scan_type"], m["duplicate_flag"] = r.u(4), r.u(2), r.u1()
            if hrd is not None and (hrd["nal"] or hrd["vcl"]):
                m["au_cpb_removal_delay_minus1"] = r.u(hrd["au_cpb_removal_delay_length_minus1"] + 1)
                m["pic_dpb_output_delay"] = r.u(hrd["dpb_output_delay_length_minus1"] + 1)
                subset(not hrd["sub_pic_hrd_params_present_flag"], "sub-picture HRD timing")
        elif ptype == 137:                                      # D.2.28 mastering_display_colour_volume
            m["primaries"] = [(r.u(16), r.u(16)) for _ in range(3)]
            m["white_point"] = (r.u(16), r.u(16))
            m["max_luminance"], m["min_luminance"] = r.u(32), r.u(32)
        elif ptype == 144:                                      # D.2.35 content_light_level_info
            m["max_content_light_level"], m["max_pic_average_light_level"] = r.u(16), r.u(16)
        elif ptype == 132:                                      # D.2.19 decoded_picture_hash (suffix SEI only)
            subset(nal_type == 40, "decoded picture hash in a prefix SEI NAL unit")
            m["hash_type"] = r.u(8)
            subset(m["hash_type"] <= 2, "hash_type %d" % m["hash_type"])
            vals = []
            for _ in range(3):                                  # cIdx 0..2 (chroma_format_idc 1)
                if m["hash_type"] == 0:
                    vals.append(bytes(r.u(8) for _ in range(16)))      # picture_md5[cIdx][i]
                else:
                    vals.append(r.u(16) if m["hash_type"] == 1 else r.u(32))   # picture_crc / picture_checksum
            m["hash"] = vals
        else:
            raise Unsupported("SEI payload type %d" % ptype)
        need(r.pos - start <= 8 * size, "SEI payload %d reads past its size" % ptype)
        if r.pos - start < 8 * size:                            # payload extension: only bit_equal_to_one + zeros allowed here
            need(r.u1() == 1, "SEI payload %d: size larger than its syntax" % ptype)
            while r.pos - start < 8 * size:
                need(r.u1() == 0, "SEI payload_bit_equal_to_zero")
        msgs.append(m)
        if not r.more_rbsp_data():
            break
    r.rbsp_trailing_bits()
    return msgs


# ================================================================ 6.5.1 / 6.5.2 / 6.5.3-6.5.5 scans and address tables
def diag_scan(blk):                                             # 6.5.3 up-right diagonal
    out, x, y = [], 0, 0
    while len(out) < blk * blk:
        while y >= 0:
            if x < blk and y < blk:
                out.append((x, y))
            y -= 1
            x += 1
        y, x = x, 0
    return out


def horiz_scan(blk):                                            # 6.5.4
    return [(i % blk, i // blk) for i in range(blk * blk)]


def vert_scan(blk):                                             # 6.5.5
    return [(i // blk, i % blk) for i in range(blk * blk)]


SCAN = {log2: [diag_scan(1 << log2), horiz_scan(1 << log2), vert_scan(1 << log2)] for log2 in range(0, 4)}   # ScanOrder[log2][scanIdx]


class Layout:
    """6.5.1 CtbAddrRsToTs / TileId / column and row boundaries, 6.5.2 MinTbAddrZs, for one SPS + PPS"""

    def __init__(self, sps, pps):
        self.ctb_log2 = sps["ctb_log2"]
        self.w, self.h = sps["width"], sps["height"]
        self.wc = (self.w + 31) >> 5
        self.hc = (self.h + 31) >> 5
        nc, nr = pps["tile_cols"], pps["tile_rows"]
        if pps["uniform_spacing_flag"]:                         # (6-3), (6-4)
            cw = [((i + 1) * self.wc) // nc - (i * self.wc) // nc for i in range(nc)]
            rh = [((j + 1) * self.hc) // nr - (j * self.hc) // nr for j in range(nr)]
        else:
            cw = pps["col_widths"] + [self.wc - sum(pps["col_widths"])]
            rh = pps["row_heights"] + [self.hc - sum(pps["row_heights"])]
        need(all(c > 0 for c in cw) and all(r_ > 0 for r_ in rh), "empty tile column or row")
        self.col_bd = [sum(cw[:i]) for i in range(nc + 1)]
        self.row_bd = [sum(rh[:j]) for j in range(nr + 1)]
        n = self.wc * self.hc
        self.rs2ts = [0] * n
        for rs in range(n):                                     # (6-5)
            tbx, tby = rs % self.wc, rs // self.wc
            tx = max(i for i in range(nc) if tbx >= self.col_bd[i])
            ty = max(j for j in range(nr) if tby >= self.row_bd[j])
            v = sum(rh[ty] * cw[i] for i in range(tx)) + sum(self.wc * rh[j] for j in range(ty))
            self.rs2ts[rs] = v + (tby - self.row_bd[ty]) * cw[tx] + tbx - self.col_bd[tx]
        self.ts2rs = [0] * n
        for rs, ts in enumerate(self.rs2ts):
            self.ts2rs[ts] = rs
        self.tile_id = [0] * n                                  # (6-7), indexed by TS address
        tid = 0
        for j in range(nr):
            for i in range(nc):
                for y in range(self.row_bd[j], self.row_bd[j + 1]):
                    for x in range(self.col_bd[i], self.col_bd[i + 1]):
                        self.tile_id[self.rs2ts[y * self.wc + x]] = tid
                tid += 1
        # (6-10) MinTbAddrZs in 4x4 units over the CTB-aligned area
        self.w4, self.h4 = self.wc << 3, self.hc << 3
        self.zs = [0] * (self.w4 * self.h4)
        for y in range(self.h4):
            for x in range(self.w4):
                v = self.rs2ts[(y >> 3) * self.wc + (x >> 3)] << 6
                for i in range(3):
                    m = 1 << i
                    v += (m * m if m & x else 0) + (2 * m * m if m & y else 0)
                self.zs[y * self.w4 + x] = v

    def tile_of_rs(self, rs):
        return self.tile_id[self.rs2ts[rs]]


# ================================================================ 9.3.4.3 arithmetic decoding engine, 9.3.2.2 context initialisation
RANGE_TAB_LPS = [                                               # Table 9-46, rangeTabLps[pStateIdx][qRangeIdx]
    (128, 176, 208, 240), (128, 167, 197, 227), (128, 158, 187, 216), (123, 150, 178, 205), (116, 142, 169, 195), (111, 135, 160, 185),
    (105, 128, 152, 175), (100, 122, 144, 166), (95, 116, 137, 158), (90, 110, 130, 150), (85, 104, 123, 142), (81, 99, 117, 135),
    (77, 94, 111, 128), (73, 89, 105, 122), (69, 85, 100, 116), (66, 80, 95, 110), (62, 76, 90, 104), (59, 72, 86, 99),
    (56, 69, 81, 94), (53, 65, 77, 89), (51, 62, 73, 85), (48, 59, 69, 80), (46, 56, 66, 76), (43, 53, 63, 72),
    (41, 50, 59, 69), (39, 48, 56, 65), (37, 45, 54, 62), (35, 43, 51, 59), (33, 41, 48, 56), (32, 39, 46, 53),
    (30, 37, 43, 50), (29, 35, 41, 48), (27, 33, 39, 45), (26, 31, 37, 43), (24, 30, 35, 41), (23, 28, 33, 39),
    (22, 27, 32, 37), (21, 26, 30, 35), (20, 24, 29, 33), (19, 23, 27, 31), (18, 22, 26, 30), (17, 21, 25, 28),
    (16, 20, 23, 27), (15, 19, 22, 25), (14, 18, 21, 24), (14, 17, 20, 23), (13, 16, 19, 22), (12, 15, 18, 21),
    (12, 14, 17, 20), (11, 14, 16, 19), (11, 13, 15, 18), (10, 12, 15, 17), (10, 12, 14, 16), (9, 11, 13, 15),
    (9, 11, 12, 14), (8, 10, 12, 14), (8, 9, 11, 13), (7, 9, 11, 12), (7, 9, 10, 12), (7, 8, 10, 11),
    (6, 8, 9, 11), (6, 7, 9, 10), (6, 7, 8, 9), (2, 2, 2, 2)]
TRANS_IDX_LPS = [0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9, 11, 11, 12, 13, 13, 15, 15, 16, 16, 18, 18, 19, 19, 21, 21, 22, 22, 23, 24,   # Table 9-47
                 24, 25, 26, 26, 27, 27, 28, 29, 29, 30, 30, 30, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 35, 36, 36, 36, 37, 37, 37, 38, 38, 63]
TRANS_IDX_MPS = [min(s + 1, 62) for s in range(63)] + [63]

# Tables 9-5 .. 9-37: initValue per ctxInc for initType 0, 1, 2 (None: the element does not occur in slices of that initType)
CTX_INIT = {
    "sao_merge_flag": ([153], [153], [153]),                    # sao_merge_left_flag and sao_merge_up_flag (Table 9-5)
    "sao_type_idx": ([200], [185], [160]),                      # sao_type_idx_luma and _chroma (Table 9-6)
    "split_cu_flag": ([139, 141, 157], [107, 139, 126], [107, 139, 126]),
    "cu_skip_flag": (None, [197, 185, 201], [197, 185, 201]),
    "pred_mode_flag": (None, [149], [134]),
    "part_mode": ([184], [154, 139, 154, 154], [154, 139, 154, 154]),
    "prev_intra_luma_pred_flag": ([184], [154], [183]),
    "intra_chroma_pred_mode": ([63], [152], [152]),
    "rqt_root_cbf": (None, [79], [79]),
    "merge_flag": (None, [110], [154]),
    "merge_idx": (None, [122], [137]),
    "inter_pred_idc": (None, [95, 79, 63, 31, 31], [95, 79, 63, 31, 31]),
    "mvp_flag": (None, [168], [168]),                           # mvp_l0_flag and mvp_l1_flag
    "split_transform_flag": ([153, 138, 138], [124, 138, 94], [224, 167, 122]),
    "cbf_luma": ([111, 141], [153, 111], [153, 111]),
    "cbf_chroma": ([94, 138, 182, 154], [149, 107, 167, 154], [149, 92, 167, 154]),   # cbf_cb and cbf_cr
    "abs_mvd_greater0_flag": (None, [140], [169]),
    "abs_mvd_greater1_flag": (None, [198], [198]),
    "last_sig_coeff_x_prefix": ([110, 110, 124, 125, 140, 153, 125, 127, 140, 109, 111, 143, 127, 111, 79, 108, 123, 63],
                                [125, 110, 94, 110, 95, 79, 125, 111, 110, 78, 110, 111, 111, 95, 94, 108, 123, 108],
                                [125, 110, 124, 110, 95, 94, 125, 111, 111, 79, 125, 126, 111, 111, 79, 108, 123, 93]),
    "coded_sub_block_flag": ([91, 171, 134, 141], [121, 140, 61, 154], [121, 140, 61, 154]),
    "sig_coeff_flag": ([111, 111, 125, 110, 110, 94, 124, 108, 124, 107, 125, 141, 179, 153, 125, 107, 125, 141, 179, 153, 125, 107, 125, 141,
                        179, 153, 125, 140, 139, 182, 182, 152, 136, 152, 136, 153, 136, 139, 111, 136, 139, 111],
                       [155, 154, 139, 153, 139, 123, 123, 63, 153, 166, 183, 140, 136, 153, 154, 166, 183, 140, 136, 153, 154, 166, 183, 140,
                        136, 153, 154, 170, 153, 123, 123, 107, 121, 107, 121, 167, 151, 183, 140, 151, 183, 140],
                       [170, 154, 139, 153, 139, 123, 123, 63, 124, 166, 183, 140, 136, 153, 154, 166, 183, 140, 136, 153, 154, 166, 183, 140,
                        136, 153, 154, 170, 153, 138, 138, 122, 121, 122, 121, 167, 151, 183, 140, 151, 183, 140]),
    "coeff_abs_level_greater1_flag": ([140, 92, 137, 138, 140, 152, 138, 139, 153, 74, 149, 92, 139, 107, 122, 152, 140, 179, 166, 182, 140, 227, 122, 197],
                                      [154, 196, 196, 167, 154, 152, 167, 182, 182, 134, 149, 136, 153, 121, 136, 137, 169, 194, 166, 167, 154, 167, 137, 182],
                                      [154, 196, 167, 167, 154, 152, 167, 182, 182, 134, 149, 136, 153, 121, 136, 122, 169, 208, 166, 167, 154, 152, 167, 182]),
    "coeff_abs_level_greater2_flag": ([138, 153, 136, 167, 152, 152], [107, 167, 91, 122, 107, 167], [107, 167, 91, 107, 107, 167]),
}
CTX_INIT["last_sig_coeff_y_prefix"] = CTX_INIT["last_sig_coeff_x_prefix"]


def init_context(init_value, qp):
    """9.3.2.2 (9-6): -> [pStateIdx, valMps]"""
    slope, offset = init_value >> 4, init_value & 15
    m, n = slope * 5 - 45, (offset << 3) - 16
    pre = min(max(1, ((m * min(max(0, qp), 51)) >> 4) + n), 126)
    mps = 1 if pre > 63 else 0
    return [pre - 64 if mps else 63 - pre, mps]


class Cabac:
    """9.3.4.3.1-9.3.4.3.5 over an RBSP held by a Bits reader; counts decoded context-coded bins per (element, ctxInc)"""

    def __init__(self, r: Bits, init_type, qp, hits):
        self.r, self.init_type, self.qp, self.hits = r, init_type, qp, hits
        self.init_contexts()
        self.start()

    def init_contexts(self):
        self.ctx = {}
        for name, per_type in CTX_INIT.items():
            vals = per_type[self.init_type]
            if vals is not None:
                self.ctx[name] = [init_context(v, self.qp) for v in vals]

    def start(self):                                            # 9.3.2.5
        self.range = 510
        self.offset = self.r.u(9)
        need(self.offset not in (510, 511), "ivlOffset 510 or 511 at initialisation")

    def decision(self, name, inc):                              # 9.3.4.3.2
        c = self.ctx[name][inc]
        self.hits[(name, inc)] += 1
        state, mps = c
        lps = RANGE_TAB_LPS[state][(self.range >> 6) & 3]
        self.range -= lps
        if self.offset >= self.range:
            b = 1 - mps
            self.offset -= self.range
            self.range = lps
            if state == 0:
                c[1] = 1 - mps
            c[0] = TRANS_IDX_LPS[state]
        else:
            b = mps
            c[0] = TRANS_IDX_MPS[state]
        while self.range < 256:                                 # 9.3.4.3.3
            self.range <<= 1
            self.offset = (self.offset << 1) | self.r.u1()
        return b

    def bypass(self):                                           # 9.3.4.3.4
        self.offset = (self.offset << 1) | self.r.u1()
        if self.offset >= self.range:
            self.offset -= self.range
            return 1
        return 0

    def bypass_bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bypass()
        return v

    def terminate(self):                                        # 9.3.4.3.5
        self.range -= 2
        if self.offset >= self.range:
            return 1                                            # no renormalisation: the last bit read is the rbsp_stop_one_bit /
        while self.range < 256:                                 # alignment_bit_equal_to_one that follows (9.3.2.5, 9.3.4.3.5)
            self.range <<= 1
            self.offset = (self.offset << 1) | self.r.u1()
        return 0

    def finish(self):
        """after a terminate bin equal to 1: the last bit the engine read must be 1 and the rest of its byte 0 (7.3.2.11 / 7.3.2.12)"""
        r = self.r
        p = r.pos
        need(p >= 1 and (r.data[(p - 1) >> 3] >> (7 - ((p - 1) & 7))) & 1 == 1, "the bit that ends the arithmetic code is not 1")
        while not r.byte_aligned():
            need(r.u1() == 0, "non-zero alignment bit after the arithmetic code")


# ================================================================ 8.5.3.2 motion data
class Mot:
    """PredFlagL0/L1, mvL0/L1, refIdxL0/L1 of one prediction block (refIdx -1 and mv 0 when the list is unused)"""
    __slots__ = ("pf", "mv", "ref")

    def __init__(self, pf=(0, 0), mv=((0, 0), (0, 0)), ref=(-1, -1)):
        self.pf, self.mv, self.ref = tuple(pf), tuple(tuple(m) for m in mv), tuple(ref)

    def key(self):
        return (self.pf, tuple(self.mv[x] if self.pf[x] else (0, 0) for x in range(2)), tuple(self.ref[x] if self.pf[x] else -1 for x in range(2)))

    def __eq__(self, o):
        return self.key() == o.key()

    def __repr__(self):
        return "Mot%r" % (self.key(),)


COMB_L0 = [0, 1, 0, 2, 1, 2, 0, 3, 1, 3, 2, 3]                 # Table 8-6 l0CandIdx / l1CandIdx by combIdx
COMB_L1 = [1, 0, 2, 0, 2, 1, 3, 0, 3, 1, 3, 2]


def clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def scale_mv(mv, td, tb):
    """8.5.3.2.8 (8-179..8-183): spatial / temporal motion vector scaling by POC distances"""
    td, tb = clip3(-128, 127, td), clip3(-128, 127, tb)
    tx = (16384 + (abs(td) >> 1)) // td if td > 0 else -((16384 + (abs(td) >> 1)) // -td)     # "/" truncates toward zero
    dsf = clip3(-4096, 4095, (tb * tx + 32) >> 6)
    out = []
    for c in mv:
        p = dsf * c
        s = 1 if p > 0 else -1 if p < 0 else 0
        out.append(clip3(-32768, 32767, s * ((abs(p) + 127) >> 8)))
    return tuple(out)


def wrap16(v):
    """(8-200..8-203): u = (mvp + mvd + 2^16) % 2^16; mv = u >= 2^15 ? u - 2^16 : u"""
    u = (v + 65536) % 65536
    return u - 65536 if u >= 32768 else u


def mpm_list(a, b):
    """8.4.2 (8-21..8-26): candModeList from candIntraPredModeA / B"""
    if a == b:
        return [0, 1, 26] if a < 2 else [a, 2 + ((a + 29) % 32), 2 + ((a - 2 + 1) % 32)]
    c = 0 if a != 0 and b != 0 else (1 if a != 1 and b != 1 else 26)
    return [a, b, c]


def luma_mode_from(prev_flag, idx, cand):
    """8.4.2 step 4"""
    if prev_flag:
        return cand[idx]
    c = sorted(cand)
    mode = idx
    for i in range(3):
        if mode >= c[i]:
            mode += 1
    return mode


def chroma_mode_from(code, luma):
    """8.4.3 Table 8-2 (4:2:0: Table 8-3 does not apply)"""
    if code == 4:
        return luma
    m = (0, 26, 10, 1)[code]
    return 34 if m == luma else m


# ================================================================ pictures
class Picture:
    def __init__(self, sps, pps, nal_type, poc):
        self.nal_type, self.poc = nal_type, poc
        w, h = sps["width"], sps["height"]
        self.w, self.h = w, h
        self.slices = []
        g = (h >> 3, w >> 3)
        self.cu = {k: np.full(g, -1, np.int32) for k in ("log2", "inter", "nxn", "skip", "merge_flag", "merge_idx", "pf0", "pf1", "mv0x", "mv0y",
                                                        "mv1x", "mv1y", "cmode", "cbf_y", "cbf_cb", "cbf_cr", "cbf_y4", "mvp0", "mvp1", "slice")}
        self.cu["imode"] = np.full(g + (4,), -1, np.int32)
        self.coef = [np.zeros((h, w), np.int32), np.zeros((h >> 1, w >> 1), np.int32), np.zeros((h >> 1, w >> 1), np.int32)]
        nctb = ((w + 31) >> 5) * ((h + 31) >> 5)
        self.sao = [None] * nctb
        self.ctb_slice = [-1] * nctb
        self.decoded = 0
        self.merge_lists = {}                                   # (x, y) -> the derived merge candidate list of an inter CU
        self.hash = None                                        # (hash_type, [3 values]) of the decoded picture hash SEI that follows it


class SliceDecoder:
    """7.3.8 slice_segment_data and everything it calls, for one slice segment"""
    sign_hiding = 0                                             # sign_data_hiding_enabled_flag of the PPS

    def __init__(self, pic: Picture, sps, pps, lay: Layout, hdr, rbsp, nal_pos, data_start, ref_pocs, hits):
        self.pic, self.sps, self.pps, self.lay, self.hdr = pic, sps, pps, lay, hdr
        self.sign_hiding = pps.get("sign_data_hiding_enabled_flag", 0)
        self.rbsp, self.nal_pos, self.data_start = rbsp, nal_pos, data_start
        self.ref_pocs = ref_pocs                                # POC of RefPicList0[0], RefPicList1[0] (None: list not in use)
        self.hits = hits
        self.w4 = lay.w4
        n4 = lay.w4 * lay.h4
        # per 4x4 state of the picture (shared by all its slices): prediction mode, CtDepth, cu_skip_flag, IntraPredModeY, motion
        if not hasattr(pic, "st_mode"):
            pic.st_mode, pic.st_depth, pic.st_skip = [None] * n4, [0] * n4, [0] * n4
            pic.st_ipm, pic.st_mot = [1] * n4, [None] * n4
        self.bd = sps["bit_depth_luma"]

    # ------------------------------------------------------------ 6.4.1 / 6.4.2 availability
    def available(self, xc, yc, xn, yn):
        lay = self.lay
        if xn < 0 or yn < 0 or xn >= lay.w or yn >= lay.h:
            return False
        zn, zc = lay.zs[(yn >> 2) * self.w4 + (xn >> 2)], lay.zs[(yc >> 2) * self.w4 + (xc >> 2)]
        if zn > zc:
            return False
        rn, rc = (yn >> 5) * lay.wc + (xn >> 5), (yc >> 5) * lay.wc + (xc >> 5)
        if self.pic.ctb_slice[rn] != self.pic.ctb_slice[rc]:   # SliceAddrRs of the slice containing each
            return False
        return lay.tile_of_rs(rn) == lay.tile_of_rs(rc)

    def pb_available(self, xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xn, yn):
        """6.4.2 prediction block availability"""
        same_cb = xcb <= xn < xcb + ncbs and ycb <= yn < ycb + ncbs
        if (npbw << 1) == ncbs and (npbh << 1) == ncbs and part_idx == 1 and ycb + npbh <= yn and xcb + npbw > xn:
            avail = False
        elif same_cb:
            avail = True
        else:
            avail = self.available(xpb, ypb, xn, yn)
        if avail and self.pic.st_mode[(yn >> 2) * self.w4 + (xn >> 2)] != "inter":
            avail = False
        return avail

    def mot_at(self, x, y):
        return self.pic.st_mot[(y >> 2) * self.w4 + (x >> 2)]

    # ------------------------------------------------------------ 8.5.3.2.2-8.5.3.2.5 merge candidates
    def merge_list(self, xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx):
        par = self.pps["log2_parallel_merge_level"]
        if par > 2 and ncbs == 8:                               # singleMCLFlag (8.5.3.2.2)
            xpb, ypb, npbw, npbh, part_idx = xcb, ycb, ncbs, ncbs, 0

        def spatial(xn, yn):
            if (xpb >> par) == (xn >> par) and (ypb >> par) == (yn >> par):
                return None
            if not self.pb_available(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xn, yn):
                return None
            return self.mot_at(xn, yn)

        # 8.5.3.2.3: the pruning compares with the neighbour whenever it is available (availableN), whether or not it became a candidate
        # (availableFlagN)
        n_a1 = spatial(xpb - 1, ypb + npbh - 1)
        n_b1 = spatial(xpb + npbw - 1, ypb - 1)
        n_b0 = spatial(xpb + npbw, ypb - 1)
        n_a0 = spatial(xpb - 1, ypb + npbh)
        a1 = n_a1
        b1 = None if n_b1 is None or (n_a1 is not None and n_b1 == n_a1) else n_b1
        b0 = None if n_b0 is None or (n_b1 is not None and n_b0 == n_b1) else n_b0
        a0 = None if n_a0 is None or (n_a1 is not None and n_a0 == n_a1) else n_a0
        b2 = None
        if sum(c is not None for c in (a0, a1, b0, b1)) != 4:
            n_b2 = spatial(xpb - 1, ypb - 1)
            if n_b2 is not None and not ((n_a1 is not None and n_b2 == n_a1) or (n_b1 is not None and n_b2 == n_b1)):
                b2 = n_b2
        lst = [c for c in (a1, b1, b0, a0, b2) if c is not None]    # (8-89) order; no temporal candidate (TMVP off)
        max_n = self.hdr["max_num_merge_cand"]
        slice_b = self.hdr["slice_type"] == 0
        orig = len(lst)
        if slice_b and 1 < orig < max_n:                        # 8.5.3.2.4 combined bi-predictive candidates
            comb = 0
            while True:
                l0, l1 = lst[COMB_L0[comb]], lst[COMB_L1[comb]]
                if l0.pf[0] and l1.pf[1] and (self.ref_poc(0, l0.ref[0]) != self.ref_poc(1, l1.ref[1]) or l0.mv[0] != l1.mv[1]):
                    lst.append(Mot((1, 1), (l0.mv[0], l1.mv[1]), (l0.ref[0], l1.ref[1])))
                comb += 1
                if comb == orig * (orig - 1) or len(lst) == max_n:
                    break
        num_ref = self.hdr["num_ref_idx"][0] if not slice_b else min(self.hdr["num_ref_idx"])
        zero = 0
        while len(lst) < max_n:                                 # 8.5.3.2.5 zero candidates
            ref = zero if zero < num_ref else 0
            lst.append(Mot((1, 1) if slice_b else (1, 0), ((0, 0), (0, 0)), (ref, ref) if slice_b else (ref, -1)))
            zero += 1
        return lst[:max_n]

    def ref_poc(self, lx, ref_idx):
        return self.ref_pocs[lx]                                # one picture per list: RefPicListX[0]

    # ------------------------------------------------------------ 8.5.3.2.6-8.5.3.2.7 AMVP
    def amvp_list(self, xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, lx):
        ly = 1 - lx
        target = self.ref_poc(lx, 0)
        cur = self.pic.poc

        def nb(xn, yn):
            if not self.pb_available(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xn, yn):
                return None
            return self.mot_at(xn, yn)

        def no_scale(m):
            if m.pf[lx] and self.ref_poc(lx, m.ref[lx]) == target:
                return m.mv[lx]
            if m.pf[ly] and self.ref_poc(ly, m.ref[ly]) == target:
                return m.mv[ly]
            return None

        def scaled(m):
            if m.pf[lx]:
                mv, rp = m.mv[lx], self.ref_poc(lx, m.ref[lx])
            elif m.pf[ly]:
                mv, rp = m.mv[ly], self.ref_poc(ly, m.ref[ly])
            else:
                return None
            return scale_mv(mv, cur - rp, cur - target)            # both short-term (no long-term pictures in the subset)

        a0, a1 = nb(xpb - 1, ypb + npbh), nb(xpb - 1, ypb + npbh - 1)
        is_scaled = a0 is not None or a1 is not None
        mva = None
        for m in (a0, a1):
            if m is not None and mva is None:
                mva = no_scale(m)
        if mva is None:
            for m in (a0, a1):
                if m is not None and mva is None:
                    mva = scaled(m)
        bs = [nb(xpb + npbw, ypb - 1), nb(xpb + npbw - 1, ypb - 1), nb(xpb - 1, ypb - 1)]
        mvb = None
        for m in bs:
            if m is not None and mvb is None:
                mvb = no_scale(m)
        if not is_scaled and mvb is not None and mva is None:
            mva = mvb                                           # (8-185): B copied to A when no A neighbour was available
        if not is_scaled:
            mvb = None
            for m in bs:
                if m is not None and mvb is None:
                    mvb = scaled(m)
        lst = []
        if mva is not None:
            lst.append(mva)
        if mvb is not None and not (mva is not None and mvb == mva):
            lst.append(mvb)
        lst = lst[:2]
        while len(lst) < 2:
            lst.append((0, 0))
        return lst

    # ------------------------------------------------------------ 7.3.8.1 slice_segment_data
    def run(self):
        h, lay, pic = self.hdr, self.lay, self.pic
        r = Bits(self.rbsp, 8 * self.data_start)
        ts = lay.rs2ts[h["slice_segment_address"]]
        init_type = 0 if h["slice_type"] == 2 else (1 if h["slice_type"] == 1 else 2)
        if h.get("cabac_init_flag") and h["slice_type"] != 2:
            init_type = 3 - init_type
        self.init_type = init_type
        cab = Cabac(r, init_type, h["slice_qp"], self.hits)
        self.cab = cab
        substream_ends = []
        n_ctb = lay.wc * lay.hc
        while True:
            rs = lay.ts2rs[ts]
            need(pic.ctb_slice[rs] < 0, "CTB %d coded twice" % rs)
            pic.ctb_slice[rs] = h["slice_addr_rs"]
            self.coding_tree_unit(rs)
            pic.decoded += 1
            end = cab.terminate()
            ts += 1
            if end:
                cab.finish()
                substream_ends.append(r.pos >> 3)
                break
            need(ts < n_ctb, "slice data continues past the last CTB")
            if self.pps["tiles_enabled_flag"] and lay.tile_id[ts] != lay.tile_id[ts - 1]:
                need(cab.terminate() == 1, "end_of_subset_one_bit is not 1")
                cab.finish()
                substream_ends.append(r.pos >> 3)
                cab.init_contexts()                             # 9.3.1: contexts and engine restart at the first CTB of a tile
                cab.start()
        # 7.3.2.9 / 7.4.3.9: rbsp_slice_segment_trailing_bits were consumed by finish(); only cabac_zero_words may follow
        rest = self.rbsp[r.pos >> 3:]
        need(len(rest) % 2 == 0 and all(b == 0 for b in rest), "bytes after the slice data that are not cabac_zero_words")
        self.cabac_zero_words = len(rest) // 2
        # 7.4.7.1 entry points: substream k starts where the offsets say, counted in NAL bytes from the first byte of the slice data
        offs = h["entry_point_offsets"]
        need(len(offs) == len(substream_ends) - 1, "num_entry_point_offsets %d for %d substreams" % (len(offs), len(substream_ends)))
        first = self.nal_pos[self.data_start]
        starts = [first] + [self.nal_pos[e] for e in substream_ends[:-1]]
        for k, o in enumerate(offs):
            need(starts[k + 1] - starts[k] == o, "entry_point_offset_minus1[%d] + 1 = %d, substream is %d bytes" % (k, o, starts[k + 1] - starts[k]))
        self.last_ts = ts - 1
        return self

    # ------------------------------------------------------------ 7.3.8.2 / 7.3.8.3
    def coding_tree_unit(self, rs):
        x, y = (rs % self.lay.wc) << 5, (rs // self.lay.wc) << 5
        if self.hdr["slice_sao_luma_flag"] or self.hdr["slice_sao_chroma_flag"]:
            self.sao(rs)
        self.coding_quadtree(x, y, 5, 0)

    def sao(self, rs):
        h, lay, pic, cab = self.hdr, self.lay, self.pic, self.cab
        rx, ry = rs % lay.wc, rs // lay.wc
        merge_left = merge_up = 0
        if rx > 0:
            if rs > h["slice_addr_rs"] and lay.tile_of_rs(rs) == lay.tile_of_rs(rs - 1):        # leftCtbInSliceSeg, leftCtbInTile
                merge_left = cab.decision("sao_merge_flag", 0)
        if ry > 0 and not merge_left:
            up = rs - lay.wc
            if up >= h["slice_addr_rs"] and lay.tile_of_rs(rs) == lay.tile_of_rs(up):              # upCtbInSliceSeg, upCtbInTile
                merge_up = cab.decision("sao_merge_flag", 0)
        if merge_left or merge_up:
            src = pic.sao[rs - 1 if merge_left else rs - lay.wc]
            pic.sao[rs] = {k: (list(v) if isinstance(v, list) else v) for k, v in src.items()}
            pic.sao[rs]["offset"] = [list(o) for o in src["offset"]]
            return
        p = {"type": [0, 0], "eo_class": [0, 0], "band_pos": [0, 0, 0], "offset": [[0] * 4 for _ in range(3)]}
        cmax = (1 << (min(self.bd, 10) - 5)) - 1
        for c in range(3):
            if (c == 0 and not h["slice_sao_luma_flag"]) or (c > 0 and not h["slice_sao_chroma_flag"]):
                continue
            if c < 2:                                           # sao_type_idx: TR cMax 2, first bin context coded, second bypass
                t = 0
                if cab.decision("sao_type_idx", 0):
                    t = 2 if cab.bypass() else 1
                p["type"][c] = t
            t = p["type"][min(c, 1)]
            if t == 0:
                continue
            absv = []
            for _ in range(4):                                  # sao_offset_abs: TR bypass, cMax (1 << (Min(bitDepth, 10) - 5)) - 1
                v = 0
                while v < cmax and cab.bypass():
                    v += 1
                absv.append(v)
            if t == 1:
                sign = [cab.bypass() if a else 0 for a in absv]
                p["band_pos"][c] = cab.bypass_bits(5)
                p["offset"][c] = [(-a if s else a) for a, s in zip(absv, sign)]       # (7-72), log2OffsetScale 0
            else:
                if c < 2:
                    p["eo_class"][c] = cab.bypass_bits(2)
                p["offset"][c] = [absv[0], absv[1], -absv[2], -absv[3]]          # 7.4.9.3.2: edge offsets 0, 1 >= 0, 2, 3 <= 0
        pic.sao[rs] = p

    # ------------------------------------------------------------ 7.3.8.4 coding_quadtree
    def coding_quadtree(self, x0, y0, log2, depth):
        lay, cab = self.lay, self.cab
        n = 1 << log2
        if x0 + n <= lay.w and y0 + n <= lay.h and log2 > 3:
            inc = 0                                             # 9.3.4.2.2 (9-35)
            if self.available(x0, y0, x0 - 1, y0) and self.pic.st_depth[(y0 >> 2) * self.w4 + ((x0 - 1) >> 2)] > depth:
                inc += 1
            if self.available(x0, y0, x0, y0 - 1) and self.pic.st_depth[((y0 - 1) >> 2) * self.w4 + (x0 >> 2)] > depth:
                inc += 1
            split = cab.decision("split_cu_flag", inc)
        else:
            split = 1 if log2 > 3 else 0
        if split:
            h = n >> 1
            for k in range(4):
                x1, y1 = x0 + (k & 1) * h, y0 + (k >> 1) * h
                if x1 < lay.w and y1 < lay.h:
                    self.coding_quadtree(x1, y1, log2 - 1, depth + 1)
        else:
            self.coding_unit(x0, y0, log2, depth)

    def fill(self, arr, x0, y0, n, v):
        w4 = self.w4
        for yy in range(y0 >> 2, (y0 + n) >> 2):
            base = yy * w4
            for xx in range(x0 >> 2, (x0 + n) >> 2):
                arr[base + xx] = v

    # ------------------------------------------------------------ 7.3.8.5 coding_unit
    def coding_unit(self, x0, y0, log2, depth):
        h, pic, cab = self.hdr, self.pic, self.cab
        n = 1 << log2
        rec = {"log2": log2, "inter": 0, "nxn": 0, "skip": 0, "merge_flag": 0, "merge_idx": -1, "pf0": 0, "pf1": 0,
               "mv0x": 0, "mv0y": 0, "mv1x": 0, "mv1y": 0, "cmode": -1, "cbf_y": 0, "cbf_cb": 0, "cbf_cr": 0, "cbf_y4": 0,
               "mvp0": -1, "mvp1": -1, "slice": h["slice_addr_rs"]}
        imodes = [-1] * 4
        self.fill(pic.st_depth, x0, y0, n, depth)
        skip = 0
        if h["slice_type"] != 2:
            inc = 0                                             # 9.3.4.2.2 (9-36)
            if self.available(x0, y0, x0 - 1, y0) and pic.st_skip[(y0 >> 2) * self.w4 + ((x0 - 1) >> 2)]:
                inc += 1
            if self.available(x0, y0, x0, y0 - 1) and pic.st_skip[((y0 - 1) >> 2) * self.w4 + (x0 >> 2)]:
                inc += 1
            skip = cab.decision("cu_skip_flag", inc)
        self.fill(pic.st_skip, x0, y0, n, skip)
        rqt_root = 1
        if skip:
            rec.update(inter=1, skip=1, merge_flag=1)
            self.fill(pic.st_mode, x0, y0, n, "inter")
            self.prediction_unit(x0, y0, n, n, x0, y0, n, 0, rec, skip=True)
            rqt_root = 0
        else:
            intra = cab.decision("pred_mode_flag", 0) if h["slice_type"] != 2 else 1
            self.fill(pic.st_mode, x0, y0, n, "intra" if intra else "inter")
            part_nxn = 0
            if not intra or log2 == 3:                          # part_mode (9.3.3.7 Table 9-43): bin 0 = 1 is PART_2Nx2N
                b0 = cab.decision("part_mode", 0)
                if intra:
                    part_nxn = 1 - b0
                else:
                    subset(b0 == 1, "inter part_mode other than PART_2Nx2N")
            if intra:
                rec["nxn"] = part_nxn
                parts = 4 if part_nxn else 1
                pb = n >> 1 if part_nxn else n
                prev = [cab.decision("prev_intra_luma_pred_flag", 0) for _ in range(parts)]
                for k in range(parts):
                    xp, yp = x0 + (k & 1) * pb, y0 + (k >> 1) * pb
                    if prev[k]:
                        idx = 0                                 # mpm_idx: TR cMax 2, bypass
                        while idx < 2 and cab.bypass():
                            idx += 1
                    else:
                        idx = cab.bypass_bits(5)                # rem_intra_luma_pred_mode: FL 5 bits
                    mode = luma_mode_from(prev[k], idx, mpm_list(self.cand_mode(xp, yp, xp - 1, yp), self.cand_mode(xp, yp, xp, yp - 1)))
                    self.fill(pic.st_ipm, xp, yp, pb, mode)
                    imodes[k] = mode
                if parts == 1:
                    imodes = [imodes[0]] * 4
                code = 4                                        # intra_chroma_pred_mode (9.3.3.8): "0" -> 4, "1" + 2 bypass bins -> 0..3
                if cab.decision("intra_chroma_pred_mode", 0):
                    code = cab.bypass_bits(2)
                rec["cmode"] = chroma_mode_from(code, imodes[0])
            else:
                rec["inter"] = 1
                self.prediction_unit(x0, y0, n, n, x0, y0, n, 0, rec, skip=False)
                if not rec["merge_flag"]:
                    rqt_root = cab.decision("rqt_root_cbf", 0)
            if intra:
                self.fill(pic.st_mot, x0, y0, n, None)
        if rqt_root:
            intra = not rec["inter"]
            max_depth = (self.sps["max_transform_hierarchy_depth_intra"] + rec["nxn"]) if intra else self.sps["max_transform_hierarchy_depth_inter"]
            self.cu_ctx = (intra, rec, imodes)
            self.transform_tree(x0, y0, x0, y0, log2, 0, 0, max_depth, rec["nxn"], [1, 1], [1, 1])
        g = pic.cu
        sl = (slice(y0 >> 3, (y0 + n) >> 3), slice(x0 >> 3, (x0 + n) >> 3))
        for k, v in rec.items():
            g[k][sl] = v
        g["imode"][sl] = imodes

    def cand_mode(self, xp, yp, xn, yn):
        """8.4.2 steps 1-2: candIntraPredModeX"""
        if not self.available(xp, yp, xn, yn):
            return 1
        i = (yn >> 2) * self.w4 + (xn >> 2)
        if self.pic.st_mode[i] != "intra":
            return 1
        if yn < yp and yn < ((yp >> 5) << 5):                   # B outside the current CTB
            return 1
        return self.pic.st_ipm[i]

    # ------------------------------------------------------------ 7.3.8.6 prediction_unit, 7.3.8.9 mvd_coding
    def prediction_unit(self, xcb, ycb, npbw, npbh, xpb, ypb, ncbs, part_idx, rec, skip):
        h, cab, pic = self.hdr, self.cab, self.pic
        max_n = h["max_num_merge_cand"]

        def merge_idx():
            i = 0
            if max_n > 1:                                       # TR cMax MaxNumMergeCand - 1, first bin context coded, the rest bypass
                if cab.decision("merge_idx", 0):
                    i = 1
                    while i < max_n - 1 and cab.bypass():
                        i += 1
            return i

        if skip:
            merge = 1
        else:
            merge = cab.decision("merge_flag", 0)
        if merge:
            idx = merge_idx()
            lst = self.merge_list(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx)
            pic.merge_lists[(xpb, ypb)] = lst
            m = lst[idx]
            if m.pf[0] and m.pf[1] and npbw + npbh == 12:       # 8.5.3.2.2: 8x4 / 4x8 bi -> L0
                m = Mot((1, 0), (m.mv[0], (0, 0)), (m.ref[0], -1))
            rec.update(merge_flag=1, merge_idx=idx)
        else:
            pic.merge_lists[(xpb, ypb)] = self.merge_list(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx)
            idc = 0                                             # PRED_L0
            if h["slice_type"] == 0:                            # inter_pred_idc (9.3.3.7, 9.3.4.2.2 Table 9-41)
                if npbw + npbh != 12:
                    if cab.decision("inter_pred_idc", self.ct_depth(xcb, ycb)):
                        idc = 2
                    else:
                        idc = cab.decision("inter_pred_idc", 4)
                else:
                    idc = cab.decision("inter_pred_idc", 4)
            pf, mv, ref = [0, 0], [(0, 0), (0, 0)], [-1, -1]
            for lx in range(2):
                if (lx == 0 and idc == 1) or (lx == 1 and idc == 0):
                    continue
                subset(h["num_ref_idx"][lx] == 1, "ref_idx_l%d present" % lx)
                if lx == 1 and h["mvd_l1_zero_flag"] and idc == 2:
                    mvd = (0, 0)
                else:
                    mvd = self.mvd_coding()
                f = cab.decision("mvp_flag", 0)
                mvp = self.amvp_list(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, lx)[f]
                pf[lx], ref[lx] = 1, 0
                mv[lx] = (wrap16(mvp[0] + mvd[0]), wrap16(mvp[1] + mvd[1]))
                rec["mvp%d" % lx] = f
            m = Mot(pf, mv, ref)
        rec.update(pf0=m.pf[0], pf1=m.pf[1])
        if m.pf[0]:
            rec.update(mv0x=m.mv[0][0], mv0y=m.mv[0][1])
        if m.pf[1]:
            rec.update(mv1x=m.mv[1][0], mv1y=m.mv[1][1])
        self.fill(pic.st_mot, xpb, ypb, npbw, m)

    def ct_depth(self, x, y):
        return self.pic.st_depth[(y >> 2) * self.w4 + (x >> 2)]

    def mvd_coding(self):
        cab = self.cab
        g0 = [cab.decision("abs_mvd_greater0_flag", 0), cab.decision("abs_mvd_greater0_flag", 0)]
        g1 = [cab.decision("abs_mvd_greater1_flag", 0) if g0[c] else 0 for c in range(2)]
        out = []
        for c in range(2):
            v = 0
            if g0[c]:
                v = 1
                if g1[c]:
                    v = 2 + self.exp_golomb_bypass(1)           # abs_mvd_minus2: EG1 (9.3.3.3)
                if cab.bypass():
                    v = -v
            out.append(v)
        return tuple(out)

    def exp_golomb_bypass(self, k):
        """9.3.3.3 k-th order Exp-Golomb, bypass bins"""
        cab = self.cab
        v = 0
        while cab.bypass():
            v += 1 << k
            k += 1
            need(k < 32, "Exp-Golomb prefix too long")
        return v + cab.bypass_bits(k)

    # ------------------------------------------------------------ 7.3.8.8 transform_tree, 7.3.8.10 transform_unit
    def transform_tree(self, x0, y0, xb, yb, log2, depth, blk, max_depth, intra_split, pcb, pcr):
        cab = self.cab
        intra, rec, imodes = self.cu_ctx
        if log2 <= 5 and log2 > 2 and depth < max_depth and not (intra_split and depth == 0):
            split = cab.decision("split_transform_flag", 5 - log2)
        else:
            inter_split = 0                                     # interSplitFlag needs a non-2Nx2N inter partition: none in the subset
            split = 1 if (log2 > 5 or (intra_split and depth == 0) or inter_split) else 0
        cbf_cb, cbf_cr = 0, 0
        if log2 > 2:
            if depth == 0 or pcb[depth - 1]:
                cbf_cb = cab.decision("cbf_chroma", depth)
            if depth == 0 or pcr[depth - 1]:
                cbf_cr = cab.decision("cbf_chroma", depth)
        elif depth > 0:                                         # 4x4 luma in 4:2:0: chroma cbf of the parent (7.4.9.8)
            cbf_cb, cbf_cr = pcb[depth - 1], pcr[depth - 1]
        pcb, pcr = pcb[:depth] + [cbf_cb], pcr[:depth] + [cbf_cr]
        if split:
            hh = 1 << (log2 - 1)
            for k in range(4):
                self.transform_tree(x0 + (k & 1) * hh, y0 + (k >> 1) * hh, x0, y0, log2 - 1, depth + 1, k, max_depth, intra_split, pcb, pcr)
            return
        if intra or depth != 0 or cbf_cb or cbf_cr:
            cbf_luma = cab.decision("cbf_luma", 1 if depth == 0 else 0)
        else:
            cbf_luma = 1
        # transform_unit
        k = ((y0 >> 2) & 1) * 2 + ((x0 >> 2) & 1) if rec["nxn"] else 0         # NxN: the PU of this 4x4 TU (8x8 CU)
        if cbf_luma:
            self.residual_coding(x0, y0, log2, 0, imodes[k] if intra else None)
        if rec["nxn"]:
            rec["cbf_y4"] |= cbf_luma << k
        rec["cbf_y"] |= cbf_luma
        if log2 > 2:
            cm = rec["cmode"] if intra else None
            if cbf_cb:
                self.residual_coding(x0, y0, log2 - 1, 1, cm)
            if cbf_cr:
                self.residual_coding(x0, y0, log2 - 1, 2, cm)
            rec["cbf_cb"] |= cbf_cb
            rec["cbf_cr"] |= cbf_cr
        elif blk == 3:
            cm = rec["cmode"] if intra else None
            if pcb[depth - 1]:
                self.residual_coding(xb, yb, 2, 1, cm)
            if pcr[depth - 1]:
                self.residual_coding(xb, yb, 2, 2, cm)
            rec["cbf_cb"] |= pcb[depth - 1]
            rec["cbf_cr"] |= pcr[depth - 1]

    # ------------------------------------------------------------ 7.3.8.11 residual_coding
    def residual_coding(self, x0, y0, log2, c, pred_mode):
        out = self.residual_block(log2, c, pred_mode)
        if c == 0:
            self.pic.coef[0][y0:y0 + (1 << log2), x0:x0 + (1 << log2)] = out
        else:
            xc, yc = x0 >> 1, y0 >> 1
            self.pic.coef[c][yc:yc + (1 << log2), xc:xc + (1 << log2)] = out

    def residual_block(self, log2, c, pred_mode):
        """the levels of one TB in raster order; pred_mode: the intra prediction mode that picks the scan, None for inter"""
        cab = self.cab
        dec = cab.decision
        byp = cab.bypass
        scan_idx = 0                                            # 7.4.9.11
        if pred_mode is not None and (log2 == 2 or (log2 == 3 and c == 0)):
            if 6 <= pred_mode <= 14:
                scan_idx = 2
            elif 22 <= pred_mode <= 30:
                scan_idx = 1
        # last_sig_coeff_{x,y}_prefix: TR cMax (log2 << 1) - 1, ctxInc = (binIdx >> ctxShift) + ctxOffset (9.3.4.2.3)
        if c == 0:
            off, shift = 3 * (log2 - 2) + ((log2 - 1) >> 2), (log2 + 1) >> 2
        else:
            off, shift = 15, log2 - 2
        cmax = (log2 << 1) - 1
        pre = []
        for name in ("last_sig_coeff_x_prefix", "last_sig_coeff_y_prefix"):
            v = 0
            while v < cmax and dec(name, (v >> shift) + off):
                v += 1
            pre.append(v)
        last = []
        for v in pre:                                           # suffix: FL (prefix >> 1) - 1 bits, bypass (7.4.9.11)
            if v > 3:
                nb = (v >> 1) - 1
                last.append((1 << nb) * (2 + (v & 1)) + cab.bypass_bits(nb))
            else:
                last.append(v)
        lx, ly = last
        if scan_idx == 2:
            lx, ly = ly, lx
        need(lx < (1 << log2) and ly < (1 << log2), "last significant position outside the TB")
        sb_scan = SCAN[log2 - 2][scan_idx]
        pos_scan = SCAN[2][scan_idx]
        nsb = 1 << (log2 - 2)
        # lastSubBlock / lastScanPos
        last_sb = next(i for i in range(len(sb_scan) - 1, -1, -1) if sb_scan[i] == (lx >> 2, ly >> 2))
        last_pos = next(p for p in range(15, -1, -1) if pos_scan[p] == (lx & 3, ly & 3))
        csbf = [[0] * nsb for _ in range(nsb)]
        out = np.zeros((1 << log2, 1 << log2), np.int32)
        g1ctx_prev = None                                       # greater1Ctx state carried between sub-blocks (9.3.4.2.6)
        first_sb = True
        for i in range(last_sb, -1, -1):
            xs, ys = sb_scan[i]
            infer_dc = 0
            if i < last_sb and i > 0:
                right = csbf[xs + 1][ys] if xs + 1 < nsb else 0
                below = csbf[xs][ys + 1] if ys + 1 < nsb else 0
                csbf[xs][ys] = dec("coded_sub_block_flag", min(right + below, 1) + (2 if c else 0))
                infer_dc = 1
            else:
                csbf[xs][ys] = 1
            sig = [0] * 16
            if i == last_sb:
                sig[last_pos] = 1
                start = last_pos - 1
            else:
                start = 15
            if csbf[xs][ys]:
                right = csbf[xs + 1][ys] if xs + 1 < nsb else 0
                below = csbf[xs][ys + 1] if ys + 1 < nsb else 0
                prev_csbf = right + (below << 1)
                for nn in range(start, -1, -1):
                    xp, yp = pos_scan[nn]
                    if nn > 0 or not infer_dc:
                        sig[nn] = dec("sig_coeff_flag", self.sig_ctx(log2, c, scan_idx, xs, ys, xp, yp, prev_csbf))
                        if sig[nn]:
                            infer_dc = 0
                    elif nn == 0 and infer_dc:
                        sig[nn] = 1                             # 7.4.9.11 inferred DC
            sig_pos = [nn for nn in range(15, -1, -1) if sig[nn]]
            if not sig_pos:
                continue
            # coeff_abs_level_greater1_flag: ctxSet and greater1Ctx (9.3.4.2.6)
            ctx_set = 0 if (i == 0 or c > 0) else 2
            if first_sb:
                last_g1 = 1
            else:
                last_g1 = g1ctx_prev
            if last_g1 == 0:
                ctx_set += 1
            first_sb = False
            g1 = {}
            g1ctx = 1
            last_g1_pos = -1
            for k, nn in enumerate(sig_pos[:8]):
                if k > 0:
                    if g1ctx > 0:
                        g1ctx = 0 if g1[sig_pos[k - 1]] else g1ctx + 1
                f = dec("coeff_abs_level_greater1_flag", ctx_set * 4 + min(3, g1ctx) + (16 if c else 0))
                g1[nn] = f
                if f and last_g1_pos < 0:
                    last_g1_pos = nn
            # the greater1Ctx the next sub-block sees: the last one derived here, updated by the last flag
            g1ctx_prev = (0 if g1[sig_pos[min(8, len(sig_pos)) - 1]] else g1ctx + 1) if g1ctx > 0 else 0
            g2 = {}
            if last_g1_pos >= 0:
                g2[last_g1_pos] = dec("coeff_abs_level_greater2_flag", ctx_set + (4 if c else 0))
            # 7.3.8.11: signHidden when lastSigScanPos - firstSigScanPos > 3 (no cu_transquant_bypass_flag in the subset); the sign of the
            # coefficient at firstSigScanPos is then not coded but inferred from the parity of sumAbsLevel (7.4.9.11)
            hidden = self.sign_hiding and sig_pos[0] - sig_pos[-1] > 3
            signs = {nn: (0 if hidden and nn == sig_pos[-1] else byp()) for nn in sig_pos}
            nsig = 0
            sum_abs = 0
            rice, last_abs, first_rem = 0, 0, True
            for nn in sig_pos:
                base = 1 + g1.get(nn, 0) + g2.get(nn, 0)
                if base == ((3 if nn == last_g1_pos else 2) if nsig < 8 else 1):
                    if not first_rem:                           # 9.3.3.11 (9-20): cRiceParam from the previous invocation
                        rice = min(rice + (1 if last_abs > 3 * (1 << rice) else 0), 4)
                    first_rem = False
                    rem = self.coeff_abs_level_remaining(rice)
                    last_abs = base + rem
                    level = base + rem
                else:
                    level = base
                sum_abs += level
                neg = signs[nn]
                if hidden and nn == sig_pos[-1] and sum_abs % 2 == 1:
                    neg = 1
                xp, yp = pos_scan[nn]
                out[(ys << 2) + yp, (xs << 2) + xp] = -level if neg else level
                nsig += 1
        return out

    def coeff_abs_level_remaining(self, rice):
        """9.3.3.11: prefix TR with cMax 4 << cRiceParam; when the prefix is all ones, suffix EG(cRiceParam + 1) of value - cMax"""
        cab = self.cab
        q = 0
        while q < 4 and cab.bypass():
            q += 1
        if q < 4:
            return (q << rice) + cab.bypass_bits(rice)
        return (4 << rice) + self.exp_golomb_bypass(rice + 1)

    @staticmethod
    def sig_ctx(log2, c, scan_idx, xs, ys, xp, yp, prev_csbf):
        """9.3.4.2.5 sig_coeff_flag ctxInc (no transform_skip_context)"""
        if log2 == 2:
            sc = CTX_IDX_MAP[(yp << 2) + xp]
        elif xs == 0 and ys == 0 and xp == 0 and yp == 0:
            sc = 0
        else:
            if prev_csbf == 0:
                sc = 2 if xp + yp == 0 else 1 if xp + yp < 3 else 0
            elif prev_csbf == 1:
                sc = 2 if yp == 0 else 1 if yp == 1 else 0
            elif prev_csbf == 2:
                sc = 2 if xp == 0 else 1 if xp == 1 else 0
            else:
                sc = 2
            if c == 0:
                if xs > 0 or ys > 0:
                    sc += 3
                if log2 == 3:
                    sc += 9 if scan_idx == 0 else 15
                else:
                    sc += 21
            else:
                sc += 9 if log2 == 3 else 12
        return sc if c == 0 else 27 + sc


CTX_IDX_MAP = [0, 1, 4, 5, 2, 3, 4, 5, 6, 6, 8, 8, 7, 7, 8]       # (9-39) ctxIdxMap


# ================================================================ 7.3.6.1 slice_segment_header
def slice_header(r: Bits, nal_type, sps_by_id, pps_by_id):
    h = {"first_slice_segment_in_pic_flag": r.u1()}
    if 16 <= nal_type <= 23:
        h["no_output_of_prior_pics_flag"] = r.u1()
    h["pps_id"] = r.ue()
    need(h["pps_id"] in pps_by_id, "slice refers to a missing PPS %d" % h["pps_id"])
    pps = pps_by_id[h["pps_id"]]
    sps = sps_by_id[pps["sps_id"]]
    lay_n = ((sps["width"] + 31) >> 5) * ((sps["height"] + 31) >> 5)
    h["slice_segment_address"] = 0
    if not h["first_slice_segment_in_pic_flag"]:
        h["slice_segment_address"] = r.u((lay_n - 1).bit_length())            # Ceil(Log2(PicSizeInCtbsY)) bits
        need(h["slice_segment_address"] < lay_n, "slice_segment_address beyond the picture")
    h["slice_addr_rs"] = h["slice_segment_address"]                           # no dependent slice segments
    for _ in range(pps["num_extra_slice_header_bits"]):
        r.u1()
    h["slice_type"] = r.ue()
    need(h["slice_type"] <= 2, "slice_type > 2")
    h["poc_lsb"], h["rps"] = 0, {"s0": [], "s1": []}
    h["short_term_ref_pic_set_sps_flag"], h["short_term_ref_pic_set_idx"] = None, None
    if nal_type not in (19, 20):
        h["poc_lsb"] = r.u(sps["log2_max_poc_lsb"])
        h["short_term_ref_pic_set_sps_flag"] = r.u1()
        nsets = len(sps["st_rps"])
        if not h["short_term_ref_pic_set_sps_flag"]:
            h["rps"] = st_ref_pic_set(r, nsets, nsets, sps["st_rps"])
        else:
            idx = r.u((nsets - 1).bit_length()) if nsets > 1 else 0
            need(idx < nsets, "short_term_ref_pic_set_idx out of range")
            h["short_term_ref_pic_set_idx"] = idx
            h["rps"] = sps["st_rps"][idx]
    h["slice_sao_luma_flag"] = h["slice_sao_chroma_flag"] = 0
    if sps["sao_enabled_flag"]:
        h["slice_sao_luma_flag"], h["slice_sao_chroma_flag"] = r.u1(), r.u1()
    h["num_ref_idx"], h["mvd_l1_zero_flag"], h["cabac_init_flag"], h["max_num_merge_cand"] = (0, 0), 0, 0, 5
    if h["slice_type"] != 2:
        h["num_ref_idx"] = pps["num_ref_idx_default"]
        if r.u1():
            h["num_ref_idx"] = (r.ue() + 1, r.ue() + 1 if h["slice_type"] == 0 else 0)
        if h["slice_type"] == 1:
            h["num_ref_idx"] = (h["num_ref_idx"][0], 0)
        subset(h["num_ref_idx"][0] == 1 and h["num_ref_idx"][1] in (0, 1), "more than one reference picture per list")
        if h["slice_type"] == 0:
            h["mvd_l1_zero_flag"] = r.u1()
        if pps["cabac_init_present_flag"]:
            h["cabac_init_flag"] = r.u1()
        h["max_num_merge_cand"] = 5 - r.ue()
        need(1 <= h["max_num_merge_cand"] <= 5, "MaxNumMergeCand outside 1..5")
    h["slice_qp_delta"] = r.se()
    h["slice_qp"] = pps["init_qp"] + h["slice_qp_delta"]
    need(-6 * (sps["bit_depth_luma"] - 8) <= h["slice_qp"] <= 51, "SliceQpY out of range")
    h["slice_cb_qp_offset"] = h["slice_cr_qp_offset"] = 0
    if pps["slice_chroma_qp_offsets_present_flag"]:
        h["slice_cb_qp_offset"], h["slice_cr_qp_offset"] = r.se(), r.se()
    override = r.u1() if pps["deblocking_filter_override_enabled_flag"] else 0
    h["slice_deblocking_filter_disabled_flag"] = pps["pps_deblocking_filter_disabled_flag"]
    if override:
        h["slice_deblocking_filter_disabled_flag"] = r.u1()
        if not h["slice_deblocking_filter_disabled_flag"]:
            h["beta_offset_div2"], h["tc_offset_div2"] = r.se(), r.se()
    h["slice_loop_filter_across_slices_enabled_flag"] = pps["loop_filter_across_slices_enabled_flag"]
    if pps["loop_filter_across_slices_enabled_flag"] and (h["slice_sao_luma_flag"] or h["slice_sao_chroma_flag"] or
                                                           not h["slice_deblocking_filter_disabled_flag"]):
        h["slice_loop_filter_across_slices_enabled_flag"] = r.u1()
    h["entry_point_offsets"], h["offset_len"] = [], None
    if pps["tiles_enabled_flag"]:
        n = r.ue()
        if n:
            h["offset_len"] = r.ue() + 1
            need(h["offset_len"] <= 32, "offset_len_minus1 > 31")
            h["entry_point_offsets"] = [r.u(h["offset_len"]) + 1 for _ in range(n)]
    r.byte_alignment()
    return h, sps, pps


# ================================================================ 8.3.1 POC, 8.3.2 RPS, 8.3.4 reference picture lists; the stream
class Stream:
    def __init__(self):
        self.vps, self.sps, self.pps = {}, {}, {}
        self.sei, self.aud, self.nal_types, self.pictures = [], [], [], []
        self.hits = collections.Counter()                       # (syntax element, ctxInc, initType) -> decoded bins


def parse_stream(stream: bytes) -> Stream:
    out = Stream()
    prev_tid0_poc = 0
    dpb = []                                                    # POCs of the pictures marked "used for reference"
    pic, lays = None, {}
    for nal in split_annexb(stream):
        hdr = (nal[0] << 8) | nal[1]                            # 7.3.1.2
        need(hdr >> 15 == 0, "forbidden_zero_bit")
        nal_type, layer, tid1 = (hdr >> 9) & 63, (hdr >> 3) & 63, hdr & 7
        need(tid1 != 0, "nuh_temporal_id_plus1 is 0")
        subset(layer == 0 and tid1 == 1, "nuh_layer_id or TemporalId other than 0")
        out.nal_types.append(nal_type)
        rbsp, nal_pos = nal_to_rbsp(nal[2:])
        nal_pos = [p + 2 for p in nal_pos]
        r = Bits(rbsp)
        if nal_type == 32:
            v = parse_vps(r)
            out.vps[v["id"]] = v
        elif nal_type == 33:
            s = parse_sps(r)
            out.sps[s["id"]] = s
        elif nal_type == 34:
            p = parse_pps(r)
            need(p["sps_id"] in out.sps, "PPS before its SPS")
            out.pps[p["id"]] = p
        elif nal_type == 35:                                    # 7.3.2.5 access_unit_delimiter_rbsp
            out.aud.append(r.u(3))
            r.rbsp_trailing_bits()
        elif nal_type in (39, 40):
            sps = next(iter(out.sps.values())) if out.sps else None
            msgs = parse_sei(r, sps, nal_type)
            out.sei.append((nal_type, msgs))
            for m in msgs:
                if m["type"] == 132:                            # D.3.19: the hash of the picture whose slices precede this suffix SEI
                    need(pic is not None and pic.hash is None, "decoded picture hash without a picture, or twice for one")
                    pic.hash = (m["hash_type"], m["hash"])
        elif nal_type in (0, 1, 19, 20):
            h, sps, pps = slice_header(r, nal_type, out.sps, out.pps)
            key = (id(sps), id(pps))
            if key not in lays:
                lays[key] = Layout(sps, pps)
            lay = lays[key]
            if h["first_slice_segment_in_pic_flag"]:
                need(pic is None or pic.decoded == len(pic.ctb_slice), "picture ended before all its CTBs were coded")
                max_lsb = 1 << sps["log2_max_poc_lsb"]
                if nal_type in (19, 20):                        # 8.3.1: IRAP with NoRaslOutputFlag = 1
                    msb = 0
                    dpb = []
                else:
                    plsb, pmsb = prev_tid0_poc & (max_lsb - 1), prev_tid0_poc - (prev_tid0_poc & (max_lsb - 1))
                    lsb = h["poc_lsb"]
                    if lsb < plsb and plsb - lsb >= max_lsb // 2:
                        msb = pmsb + max_lsb
                    elif lsb > plsb and lsb - plsb > max_lsb // 2:
                        msb = pmsb - max_lsb
                    else:
                        msb = pmsb
                poc = msb + h["poc_lsb"]
                pic = Picture(sps, pps, nal_type, poc)
                pic.layout = lay
                out.pictures.append(pic)
                # 8.3.2: every picture of the RPS must be in the DPB; the rest are no longer used for reference
                rps = h["rps"]
                before = [poc + d for d, u in rps["s0"] if u]
                after = [poc + d for d, u in rps["s1"] if u]
                all_rps = [poc + d for d, _ in rps["s0"]] + [poc + d for d, _ in rps["s1"]]
                for q in before + after:                        # 8.3.2: no "no reference picture" in RefPicSetStCurrBefore / After
                    need(q in dpb, "picture %d: the RPS names POC %d, which is not in the DPB" % (poc, q))
                dpb = [q for q in dpb if q in all_rps]
                pic.rps, pic.rps_all = (before, after), all_rps
                pic.dpb_before = list(dpb)
                if nal_type not in (0,) and tid1 == 1:          # TRAIL_N (and other sub-layer non-reference types) never become prevTid0Pic
                    prev_tid0_poc = poc
            else:
                need(pic is not None, "slice of a picture without its first slice")
                need(nal_type == pic.nal_type, "slices of one picture with different NAL types")
            need(nal_type in (19, 20) or h["poc_lsb"] == pic.poc % (1 << sps["log2_max_poc_lsb"]), "POC lsb differs between slices")
            # 8.3.4 RefPicList0 / 1 (no modification): StCurrBefore then StCurrAfter, and the reverse
            before, after = pic.rps
            ref = [None, None]
            if h["slice_type"] != 2:
                total = before + after
                need(len(total) > 0, "inter slice with an empty RPS")
                ref[0] = (before + after)[0]
                if h["slice_type"] == 0:
                    ref[1] = (after + before)[0]
            h["ref_pocs"] = tuple(ref)
            hits = collections.Counter()
            dec = SliceDecoder(pic, sps, pps, lay, h, rbsp, nal_pos, r.pos >> 3, ref, hits).run()
            init_type = dec.init_type
            for (name, inc), cnt in hits.items():
                out.hits[(name, inc, init_type)] += cnt
            pic.slices.append({"nal_type": nal_type, "slice_type": h["slice_type"], "slice_qp": h["slice_qp"], "address": h["slice_segment_address"],
                               "header": h, "cabac_zero_words": dec.cabac_zero_words, "init_type": init_type, "pps_id": h["pps_id"]})
            if h["first_slice_segment_in_pic_flag"]:
                dpb.append(pic.poc)                             # after decoding, the picture is "used for short-term reference" (8.3.2)
        else:
            raise Unsupported("NAL unit type %d" % nal_type)
    need(pic is None or pic.decoded == len(pic.ctb_slice), "the last picture ended before all its CTBs were coded")
    return out
