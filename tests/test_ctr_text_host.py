"""CPU: the strict grammar restated (tests/ctr_text_helpers.py) against `read_criteo_text`, the threshold table that stands
in for the logarithm on the device, the chunk cutter of `parse_criteo_text`, and the `reader` argument's check."""
import io

import numpy as np
import pytest

import ctr_text_helpers as th
import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import ctr_data


def assert_same(got, want):
    for g, w, name in zip(got, want, ("keys", "labels", "line_no")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


def test_restated_grammar_equals_the_host_reader_on_the_sample():
    data = open(th.SAMPLE, "rb").read()
    assert len(data) == 23948 and data.count(b"\n") == 100
    want = pkg.read_criteo_text(th.SAMPLE)
    assert want[0].shape == (100, 39)
    assert_same(th.parse_reference(data), want)


@pytest.mark.parametrize("seed,holes,final_newline", [(1, 0.0, True), (2, 0.3, True), (3, 0.3, False), (4, 1.0, True)])
def test_restated_grammar_equals_the_host_reader_on_generated_files(tmp_path, seed, holes, final_newline):
    data = th.generate_text(seed, 300, holes=holes, final_newline=final_newline)
    assert_same(th.parse_reference(data), th.host_reader(data, 13, 26, tmp_path))


def test_restated_grammar_at_other_column_counts_equals_the_padded_host_reader(tmp_path):
    data = th.generate_text(5, 200, 2, 3, holes=0.3, final_newline=False)
    got = th.parse_reference(data, 2, 3)
    assert got[0].shape[1] == 5 and 0 < got[0].shape[0] < 200
    assert_same(got, th.host_reader(data, 2, 3, tmp_path))


@pytest.mark.parametrize("line,column", [(b"1\t+5\t6\ta\tb\tc", 1), (b"1\t5\t 6\ta\tb\tc", 2), (b"1\t1_0\t6\ta\tb\tc", 1),
                                         (b"1\t5\t6\t0x1f\tb\tc", 3), (b"1\t5\t6\ta\tg1\tc", 4),
                                         (b"1\t5\t" + b"1" * 19 + b"\ta\tb\tc", 2), (b"1\t5\t6\ta\tb\t" + b"f" * 16, 5),
                                         (b"2\t5\t6\ta\tb\tc", 0), (b"\t5\t6\ta\tb\tc", 0), (b"1\t5\t6\ta\tb\tc\r", 5)])
def test_restated_grammar_refuses_what_the_header_refuses(line, column):
    good = b"0\t1\t\t1f\t\tAB\n"
    th.parse_reference(good + good, 2, 3)
    with pytest.raises(th.Refused) as e:
        th.parse_reference(good + line + b"\n" + good + b"9\t\t\t\t\t\n", 2, 3)
    assert (e.value.line, e.value.column) == (1, column)


def test_threshold_table_stands_for_the_logarithm():
    T = pkg.numeric_thresholds()
    assert T.dtype == np.int64 and T.shape == (1906,) and T[:5].tolist() == [3, 5, 6, 8, 10]
    assert (np.diff(T) > 0).all() and pkg.numeric_thresholds() is T and not T.flags.writeable
    table = T.tolist()
    for k, t in enumerate(table, 1):
        for v in range(t - 2, t + 2):
            want = ctr_data._numeric_key(str(v))
            assert want == (v - 2 if v <= 2 else int(np.searchsorted(T, v, side="right"))), (k, v)
        assert ctr_data._numeric_key(str(t)) == k and (t == 3 or ctr_data._numeric_key(str(t - 1)) == k - 1)
    rng = np.random.default_rng(0)
    for v in [int(x) for x in rng.integers(3, 1 << 62, 20000)] + list(range(-5, 20000)):
        assert ctr_data._numeric_key(str(v)) == (v - 2 if v <= 2 else int(np.searchsorted(T, v, side="right"))), v


def chunks_of(data, chunk_bytes, total=None):
    """The cutter's (chunk, final) pairs; a chunk is a view of the cutter's one buffer, so it is copied while it is valid."""
    return [(bytes(chunk), final) for chunk, final in ctr_data._cut_chunks(io.BytesIO(data).readinto, chunk_bytes, total)]


def test_cutter_cuts_after_the_last_newline_and_carries_the_tail():
    data = b"aaaa\nbb\ncccccc\ndd\n"
    assert chunks_of(data, 9) == [(b"aaaa\nbb\n", False), (b"cccccc\n", False), (b"dd\n", False)]
    assert chunks_of(data, 7) == [(b"aaaa\n", False), (b"bb\n", False), (b"cccccc\n", False), (b"dd\n", False)]
    assert chunks_of(data, 1000) == [(data, False)]
    for chunk_bytes in range(7, 30):
        for total in (None, len(data)):
            parts = chunks_of(data, chunk_bytes, total)
            assert b"".join(c for c, _ in parts) == data
            assert all(len(c) <= chunk_bytes and c.endswith(b"\n") and not final for c, final in parts)


def test_cutter_hands_the_final_unterminated_line_over_alone():
    assert chunks_of(b"aaaa\nbb\nccc", 9) == [(b"aaaa\nbb\n", False), (b"ccc", True)]
    assert chunks_of(b"aaaa\nbb\nccc", 1000) == [(b"aaaa\nbb\n", False), (b"ccc", True)]
    assert chunks_of(b"ccc", 3) == [(b"ccc", True)]
    assert chunks_of(b"ccc", 4) == [(b"ccc", True)]
    for chunk_bytes in (3, 4, 1000):
        assert chunks_of(b"ccc", chunk_bytes, total=3) == [(b"ccc", True)]
        assert chunks_of(b"a\nccc", chunk_bytes, total=5) == [(b"a\n", False), (b"ccc", True)]


def test_cutter_refuses_a_line_longer_than_a_chunk():
    assert chunks_of(b"aaaa\nbb\n", 5)[0] == (b"aaaa\n", False)
    with pytest.raises(ValueError, match="longer than chunk_bytes"):
        chunks_of(b"aaaa\nbb\n", 4)
    with pytest.raises(ValueError, match="longer than chunk_bytes"):
        chunks_of(b"bb\naaaa", 3)
    with pytest.raises(ValueError):
        chunks_of(b"a\n", 0)


def test_cutter_takes_short_reads_and_a_stream_of_unknown_length(tmp_path):
    """A pipe hands over a few bytes at a time and has no size; a path that is no regular file must not read as empty."""
    data = b"aaaa\nbb\ncccccc\ndd\nee"
    stream = io.BytesIO(data)
    parts = [(bytes(c), final) for c, final in ctr_data._cut_chunks(lambda b: stream.readinto(b[:3]), 9, None)]
    assert b"".join(c for c, _ in parts) == data and [final for _, final in parts] == [False] * (len(parts) - 1) + [True]
    assert parts[-1][0] == b"ee" and all(c.endswith(b"\n") for c, _ in parts[:-1])


def test_cutter_on_an_empty_file():
    assert chunks_of(b"", 16) == [] and chunks_of(b"", 16, total=0) == []
    assert chunks_of(b"\n", 16) == [(b"\n", False)]


def test_view_reader_reads_any_bytes_like_object_in_pieces():
    with ctr_data._ViewReader(np.frombuffer(b"aaaa\nbb\nccc", dtype=np.uint8)) as r:
        parts = [(bytes(chunk), final) for chunk, final in ctr_data._cut_chunks(r.readinto, 5, len(r.view))]
    assert parts == [(b"aaaa\n", False), (b"bb\n", False), (b"ccc", True)]


def test_an_unknown_reader_is_refused_before_anything_is_read():
    with pytest.raises(ValueError, match="reader"):
        pkg.DeviceCTRDataset.from_criteo_text(th.SAMPLE, reader="bogus")
    with pytest.raises(ValueError, match="reader"):
        pkg.DeviceCTRDataset.from_criteo_text("no such file", reader="bogus")
