"""CPU: tools/sweep.py's measurement method and output format, pinned without a device -- the mask builder against numpy, the median
rule, the case table against tools/README.md, the row lists of the uniform-width cases, and every row formatter against a line of
the profile file it once wrote (the numbers of the recorded line go in, the line comes back byte for byte)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import design_tables  # noqa: E402
import sweep  # noqa: E402


def profile_line(name, number):
    return open(os.path.join(ROOT, "profiles", name)).read().split("\n")[number - 1]


# ---- masks

def numpy_words(bits):
    return np.packbits(bits.numpy(), bitorder="little").view(np.int32)


def drawn_bits(n, density, seed, chunk_blocks):
    """what random_mask draws: one torch.rand per chunk from one seeded generator"""
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    return torch.cat([torch.rand(min(chunk_blocks, n - b0) * 1024, generator=g) < density for b0 in range(0, n, chunk_blocks)])


@pytest.mark.parametrize("density", [0.0, 1.0, 0.5])
def test_random_mask_is_numpy_packbits_of_the_same_bits(density):
    n = 8                                                    # chunks of 3, 3 and 2 blocks
    got = sweep.random_mask(n, density, 77, chunk_blocks=3, device="cpu")
    bits = drawn_bits(n, density, 77, 3) if 0.0 < density < 1.0 else torch.full((n * 1024,), density >= 1.0)
    assert got.dtype == torch.int32 and got.shape == (n * 32,)
    assert np.array_equal(got.numpy(), numpy_words(bits))
    assert int(bits.sum()) == n * 1024 * density or 3800 < int(bits.sum()) < 4400          # 0.5: 4096 +- 6 sigma of 45


def test_random_mask_every_16_keeps_only_block_0():
    n = 8
    got = sweep.random_mask(n, 0.5, 77, every=16, chunk_blocks=3, device="cpu")
    bits = drawn_bits(n, 0.5, 77, 3)
    bits[1024:] = False
    assert np.array_equal(got.numpy(), numpy_words(bits))
    assert got[:32].ne(0).any() and not got[32:].ne(0).any()


@pytest.mark.parametrize("density", [0.0, 1.0])
def test_densities_0_and_1_draw_nothing(density, monkeypatch):
    made = []
    real = torch.Generator

    def recording(*a, **kw):
        made.append(real(*a, **kw))
        return made[-1]
    monkeypatch.setattr(torch, "Generator", recording)
    sweep.random_mask(8, density, 77, chunk_blocks=3, device="cpu")
    monkeypatch.undo()
    fresh = torch.Generator(device="cpu"); fresh.manual_seed(77)
    assert len(made) == 1 and torch.equal(torch.rand(16, generator=made[0]), torch.rand(16, generator=fresh))


def test_mask_words_bit_31_is_the_sign():
    bits = torch.zeros(64, dtype=torch.bool)
    bits[31] = True
    bits[32] = True
    assert sweep.mask_words(bits).tolist() == [-(1 << 31), 1]
    assert sweep.mask_words(torch.ones(32, dtype=torch.bool)).tolist() == [-1]


# ---- medians and show

def test_median_of_an_even_length_list_is_the_upper_middle():
    assert sweep.median([4.0, 1.0, 3.0, 2.0]) == 3.0
    assert sweep.median([5.0, 1.0, 3.0]) == 3.0
    assert sweep.medians({"a": [2.0, 1.0], "b": [7.0]}) == {"a": 2.0, "b": 7.0}


def test_show_exact_string():
    assert sweep.show([0.4707, 0.4566, 0.4588]) == "   0.4588 ms (0.4566 .. 0.4707)"
    assert sweep.show([12.5, 10.0, 11.0, 13.25]) == "  12.5000 ms (10.0000 .. 13.2500)"


# ---- the case table

def test_case_table_is_what_the_readme_names():
    rows = [l for l in open(os.path.join(ROOT, "tools", "README.md")) if l.startswith("| `sweep.py --cases ")]
    named = set()
    for l in rows:
        named |= set(re.match(r"\| `sweep\.py --cases ([a-z_\\|]+)", l).group(1).replace("\\|", " ").split())
    assert named == set(sweep.CASES) and len(sweep.CASES) == 17
    assert set(re.match(r"\| `sweep\.py --cases ([a-z_\\|]+)", rows[0]).group(1).replace("\\|", " ").split()) == set(sweep.CASES)
    assert set(sweep.ROW_CASES) == {"quick", "orig", "consume", "fused", "allwidths", "widths"}
    assert sweep.TYPES == ("u32", "u64", "u16", "u8") and sweep.PEAK_GBPS == 8000


def test_unknown_case_is_an_argparse_error():
    with pytest.raises(SystemExit) as e:
        sweep.main(["--cases", "al"])
    assert e.value.code == 2


def test_row_lists():
    C = sweep.CASES
    four = ("delta", "undelta", "transpose", "untranspose")
    assert C["quick"]() == [
        ("unpack", "u32", 7), ("pack", "u32", 7), ("unfor_pack", "u32", 7), ("for_pack", "u32", 7), ("undelta_pack", "u32", 12),
        ("unpack", "u64", 17), ("pack", "u64", 17), ("unpack", "u16", 3), ("pack", "u16", 3), ("unpack", "u8", 3), ("pack", "u8", 3),
        ("undelta_pack", "u16", 9), ("undelta_pack", "u64", 20), ("undelta_pack", "u8", 4)] + [
        (op, ty, 0) for ty in ("u8", "u16", "u32", "u64") for op in four]
    assert C["orig"]() == [
        ("transpose", "u8", 0), ("untranspose", "u8", 0), ("transpose", "u16", 0), ("untranspose", "u16", 0),
        ("transpose", "u32", 0), ("untranspose", "u32", 0), ("transpose", "u64", 0), ("untranspose", "u64", 0),
        ("undelta_pack_untranspose", "u32", 12), ("undelta_pack_untranspose", "u64", 20), ("undelta_pack_untranspose", "u16", 9),
        ("undelta_pack_untranspose", "u8", 4), ("transpose_delta_pack", "u32", 12), ("transpose_delta_pack", "u64", 20),
        ("transpose_delta_pack", "u16", 9), ("transpose_delta_pack", "u8", 4)]
    assert C["consume"]() == [
        ("unpack_compare", "u32", 7), ("unpack_compare", "u32", 20), ("unpack_compare", "u64", 17), ("unpack_compare", "u16", 3),
        ("unpack_compare", "u8", 3), ("unpack_block_sums", "u32", 7), ("unpack_block_sums", "u32", 20), ("unpack_block_sums", "u64", 17),
        ("unpack_block_sums", "u16", 3), ("unpack_block_sums", "u8", 3), ("block_min_max", "u32", 0), ("block_min_max", "u64", 0),
        ("block_min_max", "u16", 0), ("block_min_max", "u8", 0)]
    assert C["fused"]() == [
        ("undelta_pack", "u32", 12), ("undelta_pack_untranspose", "u32", 12), ("transpose_delta_pack", "u32", 12),
        ("undelta_pack_untranspose", "u64", 20), ("transpose_delta_pack", "u64", 20), ("undelta_pack_untranspose", "u16", 9),
        ("transpose_delta_pack", "u16", 9), ("undelta_pack_untranspose", "u8", 4), ("transpose_delta_pack", "u8", 4)]
    widths = {"u8": (1, 2, 3, 4, 7, 8), "u16": (1, 2, 3, 4, 8, 15, 16), "u32": (1, 2, 3, 8, 16, 31, 32), "u64": (1, 2, 3, 16, 32, 63, 64)}
    assert C["widths"]() == [(op, ty, w) for ty in ("u8", "u16", "u32", "u64") for w in widths[ty] for op in ("unpack", "pack")]
    allw = C["allwidths"]()
    assert len(allw) == 7 * (8 + 16 + 32 + 64) and len(set(allw)) == len(allw)
    assert allw[:8] == [(op, "u8", 1) for op in sweep.ALLWIDTH_OPS] + [("unpack", "u8", 2)] and allw[-1] == ("transpose_delta_pack", "u64", 64)


# ---- the row formatters against recorded lines

def test_compare_columns_row_is_the_recorded_line():
    # rows 15-17 are the three medians line 16 is put in ratio to
    line = sweep.format_compare_columns_row("NEW undecided", "u32", 488281, [0.4707, 0.4588, 0.4566], 0.5676, 0.4588, 0.2368)
    assert line == profile_line("compare_columns_sweep_mixed.txt", 16)


def test_aggregate_rows_are_the_recorded_lines():
    n = 1953125
    assert sweep.format_aggregate_row("empty", "u32", n, 0, [0.7333, 0.7371, 0.7483]) == profile_line("aggregate_sweep_mixed.txt", 10)
    assert sweep.format_aggregate_row("mask=None", "u32", n, n * 1024, [1.4576, 1.4702, 1.4803]) == profile_line("aggregate_sweep_mixed.txt", 40)
    assert sweep.format_yardstick_row("aggregate call", "u32", n, [0.7783, 0.7804, 0.7905], 0.7371) == profile_line("aggregate_sweep_mixed.txt", 11)


def test_aggregate_by_rows_are_the_recorded_lines():
    n = 244140
    assert sweep.format_aggregate_by_row("u32", "4 groups", "100 %", n, [1.6933, 1.8025, 1.8605]) == profile_line("aggregate_by_sweep_mixed.txt", 4)
    assert sweep.format_yardstick_row("(a) aggregate + key unpack", "u32", n, [0.2938, 0.3051, 0.3096], 1.8025, "aggregate_by", 28) == \
        profile_line("aggregate_by_sweep_mixed.txt", 5)


def test_select_and_compare_range_rows():
    """profiles/select_sweep_mixed.txt and compare_range_sweep_mixed.txt hold no measured line yet: these two are lines the tool printed
    at 64 blocks of u16 before its cases became functions (values consistent with the printed 4-decimal figures)"""
    assert sweep.format_select_row("1 %", "u16", 64, 623, 1.0, 75840, 197000, [0.0185, 0.0194, 0.0200], 0.0192, 0.01936) == (
        "unfor_select_widths 1 %                    u16  kept  0.0095 non-empty 1.0000     0.0194 ms (min    0.0185)       3.9 GB/s 0.000     1185 B/block  "
        "x1.010 of unfor_pack_widths (0.0192 ms, 0.001)  x1.002 of compare all decided (0.0194 ms)")
    assert sweep.format_mask_offsets_row("u16", 64, [0.0396, 0.0409, 0.0450]) == "    mask_offsets u16     0.0409 ms (min 0.0396)       0.2 GB/s"
    assert sweep.format_compare_range_row("NEW undecided", "u16", 64, [0.0146, 0.0165, 0.0194], 0.01538, 0.016385) == (
        "NEW undecided                              u16     0.0165 ms (0.0146 .. 0.0194)     0.004 Gblocks/s  x1.073 of undecided, x1.007 of all decided")


def test_mixed_row_is_the_recorded_line_and_design_tables_parses_it(tmp_path):
    line = sweep.format_mixed_row("unpack_widths", "u32", 3906250, 3.5090, 24000156400)
    assert line == profile_line("r06_sweep_mixed.txt", 2)
    tail = sweep.format_mixed_row("unfor_compare_widths undecided", "u8", 64, 0.0150, 17000, "  decided 0.000")
    assert tail.endswith(" Gint/s  decided 0.000")
    (tmp_path / "mixed.txt").write_text(line + "\n" + tail + "\n")
    assert design_tables.sweep_fracs(str(tmp_path / "mixed.txt")) == {("unpack_widths", "u32"): 0.855, ("unfor_compare_widths undecided", "u8"): 0.0}


def test_allwidths_row_is_the_recorded_line():
    r = {"op": "unpack", "ty": "u8", "w": 1, "n_blocks": 6944444, "ms": 1.2668, "GBps": 6315.3, "frac": 0.7894, "Gints": 5613.6, "placed": "",
         "bare_GBps": 6731.7, "of_bare": 0.9381}
    assert sweep.format_run_row(r, wide=True) == profile_line("r06_sweep_allwidths.txt", 2)
    quick = dict(r, op="unpack", ty="u32", w=7, bare_GBps=None, of_bare=None, placed="constructed pair ABC")
    assert sweep.format_run_row(quick) == "unpack        u32  W=7   n=  6944444    1.2668 ms   6315.3 GB/s 0.789   5613.6 Gint/s   [constructed pair ABC]"
    summary = sweep.allwidths_summary([r, dict(r, w=2, frac=0.8503, of_bare=1.0023)])
    assert summary[0] == profile_line("r06_sweep_allwidths.txt", 842)
    assert summary[1] == ("# unpack                   u8   min 0.789 (W=1 )  median 0.850  max 0.850 (W=2 )   | of the bare stream of the same bytes on the same "
                          "buffers: min 0.938 (W=1 )  median 1.002")
    assert len(summary) == 4 and summary[2].startswith("# ---- the eight slowest (op, T, W): unpack u8 W=1 0.789 (0.94 of its bare stream); unpack u8 W=2")
