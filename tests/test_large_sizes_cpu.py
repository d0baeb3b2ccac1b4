"""No device: the case table of tests/large_cases.py is what its docstring table says — every size lies on the side of its limit the
case claims (the launchers' predicates restated in Python), the two sizes of a pair are adjacent, every case fits the device-memory
cap, every entry the issue names has a case — and the repeat / compare helpers are right on small numpy arrays."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import large_cases as lc

CASES = lc.CASES


def pair(stem):
    near, far = lc.BY_ID[stem + "-near"], lc.BY_ID[stem + "-far"]
    assert near.pair == far.pair == stem and near.side == "near" and far.side == "far"
    return near, far


# ---------------------------------------------------------------- the table
def test_every_pair_is_adjacent_and_differs_in_one_size():
    stems = sorted({c.pair for c in CASES if c.pair and c.run != "runner"})
    assert len(stems) >= 14
    for stem in stems:
        near, far = pair(stem)
        key, step = near.step
        assert far.sizes[key] - near.sizes[key] == step, stem          # one row, one image, or 16 columns of ldv (both multiples of 16)
        assert {k: v for k, v in near.sizes.items() if k != key} == {k: v for k, v in far.sizes.items() if k != key}, stem
        assert step == 1 or (key == "ldv" and near.sizes[key] % 16 == 0 and far.sizes[key] % 16 == 0), stem
    for model, lim in (("patch16", 65535), ("micro_vit", 65535), ("patch16h2", 32767)):
        a, b = lc.BY_ID[f"runner-{model}-{lim}"], lc.BY_ID[f"runner-{model}-{lim + 1}"]
        assert b.sizes["batch"] - a.sizes["batch"] == 1 and a.sizes["nslices"] == b.sizes["nslices"] == 1


def test_planned_gemm_sizes_lie_where_the_table_says():
    two31, two32 = 1 << 31, 1 << 32
    # out_bytes < 2^31, 16-bit output (hip:844-848): re-derived, not copied
    n, f = pair("planned-rq16-out_bytes")
    assert n.sizes["M"] == (two31 - 1) // (1536 * 2) == 699050 and 699050 * 1536 * 2 == 2147481600 and 699051 * 1536 * 2 == 2147484672
    for c in (n, f):
        s = c.sizes
        assert lc.requant_planned_route(False, s["M"], s["N"], s["K"], s["bits"]) == c.kernel
        assert (lc.gemm3_out_bytes("rq16", s["M"], s["N"]) < two31) == (c.side == "near")
        assert s["M"] * s["K"] < two32 and s["N"] * s["K"] < two32                                    # the other two terms hold on both sides
    # M * lda < 2^32 (hip:847)
    n, f = pair("planned-rq8-M_lda")
    assert n.sizes["M"] == (two32 - 1) // 384 == 11184810
    for c in (n, f):
        s = c.sizes
        assert lc.requant_planned_route(False, s["M"], s["N"], s["K"], s["bits"]) == c.kernel
        assert (s["M"] * s["K"] < two32) == (c.side == "near") and lc.gemm3_out_bytes("rq8", s["M"], s["N"]) < two31
        assert s["N"] % 32 == 0 and s["N"] == 32                       # the narrowest output gemm_as_kernel takes
    # the residual form (hip:915-918, use_gemm3's N >= 512)
    n, f = pair("planned-res16-out_bytes")
    assert n.sizes["M"] == (two31 - 1) // (512 * 2)
    for c in (n, f):
        s = c.sizes
        assert lc.residual_planned_route(False, s["M"], s["N"], s["K"]) == c.kernel
        assert (lc.gemm3_out_bytes("res16", s["M"], s["N"]) < two31) == (c.side == "near")
    assert not lc.use_gemm3(10 ** 6, 384, 384, 4) and lc.use_gemm3(10 ** 6, 512, 384, 4)


def test_qkv_scatter_sizes_lie_where_the_table_says():
    two31 = 1 << 31
    # the issue's pair is M = 5 592 405 | 5 592 406; the scatter takes whole images: 5 592 405 = 28 679 * 195, and the next image is the far side
    assert (two31 - 1) // 384 == 5592405 and 5592405 == 28679 * 195 and 5592406 == 2 * 2796203
    assert all(2796203 % d for d in range(2, 1673))                     # 2 796 203 is prime: no T <= 640 gives 5 592 406 whole images
    for stem, key in (("planned-qkv-out_bytes", "M * D"), ("planned-qkv-vT-out_bytes", "v^T")):
        for c in pair(stem):
            s = c.sizes
            M, D = s["B"] * s["T"], s["H"] * s["dh"]
            assert lc.qkv_planned_route(False, s["B"], s["T"], s["H"], s["dh"], s["ldv"]) == c.kernel
            ob = lc.gemm3_out_bytes("qkv", M, 3 * D, D, s["T"], s["ldv"])
            assert (ob < two31) == (c.side == "near") and M >= 256 and M < (1 << 23)
            if key == "v^T":
                assert ob == (s["B"] + 1) * D * s["ldv"] > M * D        # the v^T term decides
                assert s["B"] * D * s["ldv"] < two31                    # ... while the array itself is still below 2^31 bytes on both sides
            else:
                assert ob == M * D
    n, f = pair("planned-qkv-vT-out_bytes")
    assert n.sizes["ldv"] == (two31 - 1) // (3 * 384) // 16 * 16
    # B * T < 2^23 (hip:963): gemm_ps_kernel below, the launch-per-tile kernel from there on
    for c in pair("planned-qkv-BT23"):
        s = c.sizes
        assert (s["B"] * s["T"] < (1 << 23)) == (c.side == "near")
        assert lc.qkv_planned_route(False, s["B"], s["T"], s["H"], s["dh"], 0) == c.kernel
    assert pair("planned-qkv-BT23")[0].sizes["B"] * 256 == (1 << 23) - 256


def test_ws_kernel_sizes_lie_where_the_table_says():
    two31 = 1 << 31
    assert (two31 - 1) // (3 * 197 * 64) == 56775 and 56775 * 197 * 192 == 2147457600 and 56776 * 197 * 192 == 2147495424
    for ln in ("qkv", "ln-qkv"):
        for c in pair(f"ws-{ln}-BHT64"):
            s = c.sizes
            ok = lc.qkv_ws_ok(True, 192, 576, s["B"], s["T"], s["H"], s["dh"], 0)
            assert ok == (c.side == "near") == (s["B"] * s["H"] * s["T"] * 64 < two31) and s["B"] * s["T"] < (1 << 26)
            assert c.kernel == ("gemm_ws_qkv_kernel" if ok else ("IVIT_ERR_UNSUPPORTED" if s["ln"] else lc.qkv_planned_route(True, s["B"], 197, 3, 64, 0)))
        n, f = pair(f"ws-{ln}-BH64ldv")
        assert n.sizes["ldv"] == (two31 - 1) // (192 * 1024) // 16 * 16 == 10912 and f.sizes["ldv"] == 10928
        for c in (n, f):
            s = c.sizes
            ok = lc.qkv_ws_ok(True, 192, 576, s["B"], s["T"], s["H"], s["dh"], s["ldv"])
            assert ok == (c.side == "near") == (s["B"] * s["H"] * 64 * s["ldv"] < two31) and s["B"] * s["H"] * s["T"] * 64 < two31
            assert c.kernel == ("gemm_ws_qkv_kernel" if ok else ("IVIT_ERR_UNSUPPORTED" if s["ln"] else lc.qkv_planned_route(True, 1024, 197, 3, 64, s["ldv"])))
    # B * T < 2^26 (hip:764) is implied by the term above it: at B * T = 2^26 even one head is 2^32 bytes
    assert (1 << 26) * 1 * 64 >= two31
    # K = 384 has no v^T form on this kernel, whatever the size (hip:766)
    assert not lc.qkv_ws_ok(True, 384, 1152, 1, 197, 6, 64, 208) and lc.qkv_ws_ok(True, 384, 1152, 1, 197, 6, 64, 0)


def test_unpredicated_cases_pass_the_32_bit_lines():
    """the last row's output offset is beyond 2^31 elements; a 16- or 32-bit operand's byte offset beyond 2^32"""
    two31, two32 = 1 << 31, 1 << 32
    s = lc.BY_ID["requant_i32-scalar"].sizes
    assert s["rows"] * s["C"] == (1 << 30) + 4099 and (s["rows"] * s["C"] - 1) * 4 > two32 and s["C"] % 8 != 0
    s = lc.BY_ID["requant_i32-vec8"].sizes
    assert (1 << 30) + 4099 <= s["rows"] * s["C"] < (1 << 30) + 4099 + 8 and s["C"] % 8 == 0 and (s["rows"] * s["C"] - 8) * 4 > two32
    for cid in ("quantize_input_f32", "widen_i8_i16"):
        assert lc.BY_ID[cid].sizes["n"] - 1 > two31 and lc.BY_ID[cid].sizes["n"] % 4 == 3            # a tail that is no whole vector
    for cid, width, item in (("layernorm_requant-384", 384, 2), ("shiftgelu_lut-1536", 1536, 1), ("shiftgelu_lut-16", 16, 1),
                             ("shiftmax-197-8", 197, 2), ("shiftmax-197-16", 197, 2)):
        rows = lc.BY_ID[cid].sizes["rows"]
        assert (rows - 1) * width > two31 and (item == 1 or (rows - 1) * width * item > two32), cid
        assert rows % 8 and rows % lc.BY_ID[cid].period, cid                                       # a partial tile of the kernel and of the block
    s = lc.BY_ID["layernorm_tokenorder-96"].sizes
    assert (s["B"] * s["L"] - 1) * s["C"] > two31 and (s["B"] * s["L"] - 1) * s["C"] * 2 > two32 and s["B"] % 5 and (s["B"] * s["L"]) % 96
    assert lc.shiftgelu_lut_route(1536) == "shiftgelu_lut2_kernel<3>" and lc.shiftgelu_lut_route(16) == "shiftgelu_lut2_kernel<1>"
    assert lc.shiftgelu_lut_route(3088) == "shiftgelu_lut_kernel"
    for cid, kern in (("linear_requant-gemm_nt", "gemm_nt_kernel"), ("linear_requant-gemm2", "gemm_glds_kernel"), ("linear_residual-wreg", "gemm_wreg_kernel")):
        c = lc.BY_ID[cid]
        s = c.sizes
        assert lc.linear_route(s["M"], s["N"], s["K"]) == kern == c.kernel
        bits = s.get("bits", 16)
        assert (s["M"] - 1) * s["N"] > two31 if bits == 8 else (s["M"] - 1) * s["N"] * 2 > two32, cid
        assert s["M"] % 128 and s["M"] % c.period
    s = lc.BY_ID["attention_fused-197"].sizes
    assert (s["B"] * s["H"] * s["T"] - 1) * 64 > two31 and (s["B"] * s["T"] - 1) * s["H"] * 64 > two31          # the last q row, the last ctx row
    assert s["B"] == 56776 and s["B"] % 5 and s["ldv"] % 16 == 0 and s["ldv"] >= s["T"]
    for shift in (0, 3):
        s = lc.BY_ID[f"window_attention-56-shift{shift}"].sizes
        assert s["B"] == -(-two31 // (56 * 56 * 288)) == 2378 and s["B"] * 56 * 56 * 288 > two31 and s["B"] % 3 and s["shift"] == shift
    for cid, C in (("mlp_fused_planned-192", 192), ("swin_mlp_fused-96", 96), ("ws-ln-requant-past", 192)):
        assert (lc.BY_ID[cid].sizes["M"] - 1) * C * 2 > two32 and lc.BY_ID[cid].sizes["M"] % 16, cid
    s = lc.BY_ID["ws-res-ln-past"].sizes
    assert (s["M"] - 1) * 384 * 2 > two31 and lc.ws_plan_ok(True, 384, s["M"]) and lc.ws_plan_ok(True, 192, lc.BY_ID["ws-ln-requant-past"].sizes["M"])


def test_the_65535_cases_lie_where_the_table_says():
    for c in pair("im2col-B"):
        s = c.sizes
        assert lc.im2col_route(s["B"], s["Cin"], s["HW"], s["P"]) == c.kernel and (s["B"] <= 65535) == (c.side == "near")
    for c in pair("patch_embed-B"):
        s = c.sizes
        assert lc.patch_embed_ok(s["B"], 1, 2, s["D"], 768) == (c.side == "near") == (c.kernel != "IVIT_ERR_UNSUPPORTED")
    for c in pair("embed_finish-B"):
        assert lc.embed_finish_ok(c.sizes["B"], c.sizes["T"], c.sizes["D"]) == (c.side == "near") == (c.kernel != "IVIT_ERR_INVALID")
    for c in pair("attn_qk-BH"):
        assert lc.batched_ok(c.sizes["BH"]) == (c.side == "near") == (c.kernel != "IVIT_ERR_UNSUPPORTED")
    for layout in ("tokens", "grid"):
        assert lc.BY_ID[f"hidden_f32-{layout}"].sizes["batch"] == 70001 > 65535
    assert lc.max_slice_images(True, 6) == 65535 and lc.max_slice_images(False, 2) == 32767 and lc.max_slice_images(False, 1) == 65535
    for model in lc.RUNNER_MODELS:
        for c in (x for x in CASES if x.run == "runner" and x.sizes["model"] == model):
            per_slice = -(-c.sizes["batch"] // c.sizes["nslices"])
            s = lc.RUNNER_MODELS[model]
            lim = 65535 if s is None else lc.max_slice_images(s["D"] // s["heads"] == 64, s["heads"])
            assert lim == c.sizes["limit"] and (per_slice <= lim) == (c.kernel == "forward"), c.id
    assert lc.BY_ID["runner-patch16h2-32768"].sizes["limit"] == 32767              # two heads of 32: 65535 // 2 (image, head) matrices
    # a launch holds fewer than 2^32 work-items: the pairs sit on the two sides, re-derived
    n, f = pair("shiftmax-work_items")
    assert n.sizes["rows"] == ((1 << 32) // 256 - 1) * 4 and lc.launch_fits((n.sizes["rows"] + 3) // 4, 256) and not lc.launch_fits((f.sizes["rows"] + 3) // 4, 256)
    n, f = pair("layernorm-work_items")
    assert n.sizes["rows"] == ((1 << 32) // 256 - 1) * 8 and lc.launch_fits((n.sizes["rows"] + 7) // 8, 256) and not lc.launch_fits((f.sizes["rows"] + 7) // 8, 256)
    b = lc.BY_ID["logits_topk-work_items-far"].sizes["batch"]
    assert not lc.launch_fits((b + 3) // 4, 256) and lc.launch_fits((b + 2) // 4, 256)
    r = lc.BY_ID["shiftgelu_lut-16"].sizes["rows"]
    assert not lc.launch_fits((r + 7) // 8, 256) and lc.launch_fits(((1 << 25) + 7) // 8, 256)      # one launch would not fit; a range of 2^25 rows does


def test_left_out_limits_have_the_two_sides_the_table_says():
    for name, inside, last, first in lc.LEFT_OUT:
        assert first - last == 1 and inside(last) and not inside(first), name


def test_every_case_fits_the_cap_and_every_named_entry_has_a_case():
    assert lc.CAP_BYTES == 12 * (1 << 30)
    for c in CASES:
        assert 0 < c.bytes <= lc.CAP_BYTES, (c.id, c.bytes)
        assert c.run != "runner" and sum(c.arrays.values()) > 0 or c.run == "runner"
    have = {c.entry for c in CASES}
    assert set(lc.ENTRIES_NAMED) <= have, set(lc.ENTRIES_NAMED) - have
    # the planned entries on launch_gemm3 each have a near / far pair; 8 and 16 bits of the plain form
    paired = {(c.entry, c.sizes.get("bits")) for c in CASES if c.pair}
    assert {("ivit_linear_i8_requant_planned", 8), ("ivit_linear_i8_requant_planned", 16), ("ivit_linear_i8_requant_residual_planned", None),
            ("ivit_linear_i8_qkv_planned", None), ("ivit_layernorm_linear_i8_qkv_ldv_planned", None)} <= paired
    # every C entry of a case is declared in the header
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read() + open(os.path.join(ROOT, "include", "ivit_hidden.h")).read()
    for e in have:
        assert re.search(r"\b%s\(" % e, hdr), e
    # the GPU file has a body for every `run` of the table
    src = open(os.path.join(ROOT, "tests", "test_large_sizes_gpu.py")).read()
    for run in {c.run for c in CASES}:
        assert 'lc.ids("%s")' % run in src, run


def _body(src, start):
    """the text of the function that begins with `start`, up to the first line that is a closing brace in column 0"""
    i = src.index(start)
    return src[i:src.index("\n}\n", i)]


def test_the_restated_predicates_stand_in_the_launchers():
    """every predicate large_cases.py restates is found, as text, in the function the table names for it"""
    hip = open(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_hip.hip")).read()
    model = open(os.path.join(ROOT, "i-vit_amd", "csrc", "ivit_model.h")).read()
    line = lambda start: hip[hip.index(start):hip.index("\n", hip.index(start))]
    assert "M < (1 << 26)" in line("static inline bool ws_plan_ok(")
    ws = _body(hip, "static inline bool qkv_ws_ok(")
    for text in ("B * H * T * 64 < (1ll << 31)", "B * T < (1ll << 26)", "B * H * 64 * ldv < (1ll << 31)"):
        assert text in ws, text
    g3 = _body(hip, "static int launch_gemm3(")
    for text in ("a.M * a.lda < (1LL << 32)", "a.N * a.ldb < (1LL << 32)", "out_bytes < (1LL << 31)", "(a.M / (a.T > 0 ? a.T : 1) + 1) * a.D * a.ldv"):
        assert text in g3, text
    assert "nb > 65535" in _body(hip, "static int launch_gemm(")
    assert "(a.K % 32) == 0 && a.K >= 64" in line("static inline bool use_gemm2(")
    assert "B * T < (1 << 23)" in _body(hip, "int ivit_linear_i8_qkv_planned(")
    assert "M < (1 << 26)" in _body(hip, "int ivit_linear_i8_requant_residual_layernorm_planned(")
    im = _body(hip, "int ivit_im2col_patch(")
    assert "B <= 65535" in im and "B * (H / P)" in im
    assert "B <= 65535" in _body(hip, "int ivit_embed_finish(")
    pe = _body(hip, "int ivit_patch_embed(")
    assert "B * np >= (1ll << 30)" in pe and "B > 65535" in pe and "T * D / 8 >= (1 << 22)" in pe
    assert "std::min(batch, 65535)" in _body(hip, 'extern "C" int ivit_hidden_f32(')
    assert "blocks * threads < (1LL << 32)" in _body(hip, "static inline int launch_fits(")
    assert "rows_per_launch = (int64_t)1 << 25" in _body(hip, "int ivit_shiftgelu_requant_lut(")
    for entry, guard in (("int ivit_shiftmax(", "REQUIRE_LAUNCH(h, (rows + 3) / 4, 256, 4)"), ("int ivit_shiftmax_masked(", "REQUIRE_LAUNCH(h, (rows + 3) / 4, 256, 4)"),
                         ("int ivit_shiftgelu(", "REQUIRE_LAUNCH(h, (rows + 3) / 4, 256, 4)"), ("int ivit_shiftgelu_requant(", "REQUIRE_LAUNCH(h, (rows + 3) / 4, 256, 4)"),
                         ("int ivit_layernorm(", "REQUIRE_LAUNCH(h, (rows + 7) / 8, 256, 8)"), ("int ivit_layernorm_requant(", "REQUIRE_LAUNCH(h, (rows + 7) / 8, 256, 8)"),
                         ("int ivit_layernorm_tokenorder_requant(", "REQUIRE_LAUNCH(h, (rows + LNT_ROWS - 1) / LNT_ROWS, 256, LNT_ROWS)"),
                         ("int ivit_patch_norm_tokenorder(", "REQUIRE_LAUNCH("), ("int ivit_layernorm_tokenorder(", "REQUIRE_LAUNCH("),
                         ("int ivit_logits_topk(", "REQUIRE_LAUNCH(h, (batch + 3ll) / 4, 256, 4)"), ("int ivit_logits_score(", "REQUIRE_LAUNCH("),
                         ('extern "C" int ivit_features_f32(', "REQUIRE_LAUNCH("), ('extern "C" int ivit_attention_cls_probs(', "REQUIRE_LAUNCH("),
                         ('extern "C" int ivit_class_map(', "REQUIRE_LAUNCH("), ('extern "C" int ivit_attention_map_f32(', "REQUIRE_LAUNCH("),
                         ('extern "C" int ivit_gather_rows_i16(', "REQUIRE_LAUNCH("), ("static int launch_attn2(", "REQUIRE_LAUNCH(h, BH, ATT_WAVES * 64, 1)")):
        assert guard in _body(hip, entry), entry
    assert "REQUIRE_LAUNCH(h, (rows + rpb - 1) / rpb, LNR_THREADS(S), rpb)" in hip        # the register LayerNorm's launch macro
    assert "m->fused_attention ? 65535 : 65535 / m->cfg.num_heads" in _body(model, "inline int max_slice_images(const ivit_vit_s")
    assert "Bmax > max_slice_images(m)" in _body(model, "int run_slices(")
    hdr = open(os.path.join(ROOT, "include", "ivit.h")).read()
    assert "2^32 work-items" in hdr and "67 108 860" in hdr and "at most 65535 images" in hdr


# ---------------------------------------------------------------- the helpers, on numpy
def _block(p, W, dtype=np.int16, seed=0):
    return np.random.default_rng(seed).integers(-30000, 30000, (p, W)).astype(dtype)


@pytest.mark.parametrize("p,W,M", [(7, 3, 100), (7, 3, 7), (7, 3, 5), (13, 1, 1000), (5, 8, 5 * 40), (4099, 2, 3 * 4099 + 17)])
def test_repeat_rows(p, W, M):
    b = _block(p, W)
    out = lc.repeat_rows(np, b, M)
    assert out.shape == (M, W) and out.dtype == b.dtype
    assert np.array_equal(out, b[np.arange(M) % p])


def test_repeat_rows_of_images():
    b = np.random.default_rng(1).integers(-128, 128, (3, 2, 4, 4), dtype=np.int8)
    out = lc.repeat_rows(np, b, 8)
    assert out.shape == (8, 2, 4, 4) and np.array_equal(out, b[np.arange(8) % 3])


@pytest.mark.parametrize("chunk", [1, 64, 1000, 1 << 20])
def test_first_mismatch_finds_the_planted_byte(chunk):
    """a period that does not divide M; a single differing byte in the last partial repeat, and elsewhere; the row is named"""
    p, W, M = 7, 5, 7 * 13 + 4
    b = _block(p, W)
    good = lc.repeat_rows(np, b, M)
    assert lc.first_mismatch(np, good, b, chunk) is None
    for row, col in ((M - 1, W - 1), (M - 3, 0), (7 * 13, 2), (0, 0), (7 * 6 + 3, 4), (7 * 13 - 1, 4)):
        bad = good.copy()
        bad.view(np.uint8).reshape(M, W * 2)[row, 2 * col] ^= 0x10                                  # one byte
        assert lc.first_mismatch(np, bad, b, chunk) == row, (row, col)
    two = good.copy()
    two[60, 1] += 1
    two[20, 3] += 1
    assert lc.first_mismatch(np, two, b, chunk) == 20                                               # the FIRST differing row
    short = lc.repeat_rows(np, b, 3)                                                                # fewer rows than a period
    assert lc.first_mismatch(np, short, b, chunk) is None
    short[2, 4] += 1
    assert lc.first_mismatch(np, short, b, chunk) == 2


def test_first_mismatch_refuses_another_type_or_width():
    b = _block(7, 5)
    with pytest.raises(AssertionError):
        lc.first_mismatch(np, lc.repeat_rows(np, b, 20).astype(np.int32), b)
    with pytest.raises(AssertionError):
        lc.first_mismatch(np, lc.repeat_rows(np, b, 20)[:, :4], b)


def test_all_equal_to_and_the_message():
    a = np.full(1000, lc.FILL, np.uint8)
    assert lc.all_equal_to(np, a, lc.FILL, 64)
    a[999] = 0
    assert not lc.all_equal_to(np, a, lc.FILL, 64)
    text = lc.where_it_is(5592406, 384, 2)
    assert "2^31 elements at row 5592406" in text and "2^32 bytes at row 5592406" in text
