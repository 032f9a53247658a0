"""The designed JPEG streams of tests/jpeg_stream_cases.py on the CPU: every valid case must come back from the oracle
(oracle/lf_oracle_jpeg.c) and from the product's host decoder (lane_slam_amd/csrc/jpeg_entropy.cpp through
tests/hostsim/jpeg_host.cpp) as exactly the blocks it was written from; every refused case must be refused by both with the designed
status; every case's census -- the property it was built for -- must hold; and the catalogue's copy of k_jhuff.hip's thresholds must
still be what the kernel's text says.  tests/test_gpu_jpeg_streams.py then holds the device decoder to the oracle's pixels."""
import io
import os
import re

import numpy as np
import pytest

import jpeg_stream_cases as C
from test_jpeg_host import _coefs, host  # noqa: F401  (the fixture that builds tests/hostsim/jpeg_host.cpp)

HERE = os.path.dirname(os.path.abspath(__file__))

# the catalogue the issue asks for, by name: a case that goes missing fails here, not silently
REQUIRED = """long_symbol_across_subsequence long_symbol_across_dword all_codes_16_bits codes_of_9_and_10_bits one_bit_tables
identical_tables_420 luma_on_table_1_chroma_on_0 three_components_three_tables no_dht_annex_k_tables quantiser_16_bit
dc_differences_of_2047 all_63_ac_no_eob three_zrl_then_run_14 four_zrl_end_the_block flat_420_standard_tables flat_420_one_bit_tables
flat_gray_standard_tables flat_gray_one_bit_tables gray_noise_sup_above_1 restart_1_gray_strip_2100 intervals_of_exact_lengths
restart_numbers_wrap_444 restart_1_420_600_intervals dc_carry_at_wave_boundaries dc_carry_inside_a_wave restart_larger_than_the_picture
clean_scan_beyond_lds_listed just_above_2048_subsequences raw_scan_above_64k raw_scan_above_93k flat_160_for_the_long_batch
ff00_split_by_a_chunk ffdn_split_by_a_chunk ff00_split_by_the_rounds ffdn_split_by_the_rounds runs_of_ff00 ff_is_the_last_data_byte
scan_shorter_than_a_subsequence scan_of_one_byte data_after_the_last_mcu_is_ignored refused_run_plus_size_past_63 refused_dc_symbol_12
refused_no_code_matches refused_interval_one_block_short refused_dropped_rst refused_misnumbered_rst refused_eight_padding_bits
refused_fill_byte_before_rst refused_truncated_last_interval unsupported_luma_1x2 unsupported_luma_4x1
unsupported_non_interleaved_scan""".split()


def test_the_catalogue_is_complete():
    assert sorted(REQUIRED) == sorted(C.NAMES)


def test_thresholds_are_the_kernels():
    """jpeg_stream_cases.py aims its cases with its own copy of k_jhuff.hip's constants: a retuned kernel must fail here."""
    with open(os.path.join(HERE, "..", "lane_slam_amd", "csrc", "k_jhuff.hip")) as f:
        src = f.read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) >= 1, pattern
        assert len(set(m)) == 1, (pattern, m)
        return m[0]
    assert int(one(r"#define LF_JH_SB (\d+)")) == C.JH_SB and "constexpr int JH_SB = LF_JH_SB;" in src
    assert int(one(r"#define LF_JH_THREADS (\d+)")) == C.JH_TD and "constexpr int JH_TD = LF_JH_THREADS;" in src
    assert int(one(r"constexpr int JH_T = (\d+);\s+// k_jh_unstuff")) == C.JH_T
    assert int(one(r"constexpr int JH_DL = (\d+);")) == C.JH_DL
    a, b = one(r"constexpr int JH_LDS_CLEAN = (\d+) \* (\d+);")
    assert int(a) * int(b) == C.JH_LDS_CLEAN
    assert int(one(r"base \+= \(uint32_t\)NT \* (\d+)u")) == C.JH_CHUNK
    assert {int(x) for x in re.findall(r"c0 = base \+ \(uint32_t\)t \* (\d+)u|c0 \+ (\d+)u", src) for x in x if x} == {C.JH_CHUNK}
    assert {int(x) for x in re.findall(r"u_nblk\[\w+\] = \(pn >> 16\) & (\d+)u", src)} == {C.NBLK_FIELD_MAX}
    assert "i + ((i >> 7) << 2)" in src                            # the padded raw layout: one dword per 128 bytes
    # the launch's choice between the decoder's own unstuffing and k_jh_unstuff, as Stream.unstuffs_in_decoder restates it
    assert "int lds_raw = (int)(max_scan_len + max_scan_len / 32 + 64 + 15) & ~15;" in src
    assert "int lds = (int)(max_scan_len + 64 + (max_scan_len + 64) / 32 + 32 + 15) & ~15;" in src
    assert "(I->clean_len + 48) + (I->clean_len + 48) / 32 + 16 <= lds_clean_bytes" in src


def test_census(capsys):
    """What every case was built for, as a table (pytest -s shows it), every row asserted."""
    with capsys.disabled():
        print("\n" + C.census_table())
    failed = [(n, r[0], r[1]) for n in C.NAMES for r in C.get(n).census if not r[2]]
    assert not failed, failed
    assert all(C.get(n).census for n in C.NAMES)
    # no legal stream completes more blocks in a subsequence than the 8-bit field holds: a block is at least a DC code and an EOB
    # of one bit each, which is what the 1-bit tables write
    assert C.JH_SB * 8 // 2 <= C.NBLK_FIELD_MAX


@pytest.mark.parametrize("name", C.valid_names())
def test_valid_case_decodes_to_the_designed_blocks(host, name):  # noqa: F811
    from oracle.oracle import jpeg_coefficients
    c = C.get(name)
    ref = jpeg_coefficients(c.data)
    assert ref.shape == c.expect.shape and np.array_equal(ref, c.expect), name
    rc, dense, _, n_entries = _coefs(host, c.data)
    assert rc == 0, name
    assert dense.shape == c.expect.shape and np.array_equal(dense, c.expect), name
    assert n_entries == int(np.count_nonzero(c.expect))


@pytest.mark.parametrize("name", C.IN_RANGE)
def test_in_range_case_equals_pillow(name):
    """Where the coefficients keep the samples in range the oracle's pixels are libjpeg-turbo's.  (Out of range they need not be:
    libjpeg-turbo's SIMD inverse DCT saturates, the C code wraps through the 1 024-entry range-limit table, which the oracle and
    k_jpeg.hip restate -- DESIGN.md section 8.)"""
    Image = pytest.importorskip("PIL.Image")
    from oracle.oracle import jpeg_decode
    c = C.get(name)
    assert c.in_range, name
    pil = np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB"))[..., ::-1]
    assert np.array_equal(jpeg_decode(c.data), pil), name


def test_every_in_range_case_is_compared_with_pillow():
    assert set(C.IN_RANGE) == {n for n in C.valid_names() if C.get(n).in_range}


def test_out_of_range_blocks_differ_from_pillow():
    """The fact as it stands: +-1023 everywhere at quantiser 1 decodes differently in Pillow's libjpeg-turbo (saturating SIMD IDCT)
    and in the oracle (jidctint.c's wrap through the range-limit table), so such cases are held to the oracle alone."""
    Image = pytest.importorskip("PIL.Image")
    from oracle.oracle import jpeg_decode
    c = C.get("raw_scan_above_64k")
    pil = np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB"))[..., ::-1]
    assert not np.array_equal(jpeg_decode(c.data), pil)


@pytest.mark.parametrize("name", C.refused_names())
def test_refused_case_is_refused_by_oracle_and_host(host, name):  # noqa: F811
    import ctypes
    from oracle import oracle
    c = C.get(name)
    assert _coefs(host, c.data)[0] == c.status, name
    lib = oracle._jpeg_lib()
    buf = np.frombuffer(c.data, np.uint8)
    out = np.zeros((c.rows, c.cols, 3), np.uint8)
    assert lib.lfo_jpeg_decode(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.size), out.ctypes.data_as(ctypes.c_void_p)) == c.status, name
    with pytest.raises(ValueError):
        oracle.jpeg_decode(c.data)


@pytest.mark.parametrize("name", [n for n in C.refused_names() if n in ("refused_fill_byte_before_rst", "refused_misnumbered_rst")])
def test_pillow_accepts_what_the_product_refuses(name):
    """Two deviations from libjpeg-turbo, recorded as they stand: a fill byte before RSTn (FF FF Dn, legal by
    T.81 B.1.1.2) and a wrong RSTn number are refused by the oracle, the host decoder and the device; Pillow decodes both."""
    Image = pytest.importorskip("PIL.Image")
    c = C.get(name)
    assert c.pillow_accepts and c.status == C.ERR_DECODE
    img = np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB"))
    assert img.shape == (c.rows, c.cols, 3)
