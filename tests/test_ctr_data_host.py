"""CPU: the Criteo text reader, the restated vocabulary rule against the reference mapper's output
(tests/golden/ctr_data_vocab.npz, written by gen_golden_ctr_data.py), the restated shuffle p(j), and the argument errors
of the device dataset / loader that need no device."""
import numpy as np
import pytest
import torch

import ctr_data_helpers as ch
import recsys_benchmark_amd as pkg
from recsys_benchmark_amd import ctr_data


@pytest.fixture(scope="module")
def sample():
    return pkg.read_criteo_text(ch.SAMPLE)


@pytest.fixture(scope="module")
def golden():
    return np.load(ch.GOLDEN + "/ctr_data_vocab.npz")


def test_reader_on_the_sample(sample, golden):
    keys, labels, line_no = sample
    assert keys.shape == (100, 39) and keys.dtype == np.int64
    assert labels.shape == (100,) and labels.dtype == np.uint8 and set(labels.tolist()) <= {0, 1}
    assert np.array_equal(line_no, np.arange(100)) and np.array_equal(line_no, golden["line_no"])
    assert np.array_equal(labels, golden["rows_t1"][:, 0])
    with open(ch.SAMPLE) as f:
        lines = [line.rstrip("\n").split("\t") for line in f]
    text = np.array([v[1:] for v in lines])
    assert np.array_equal(keys[:, :13] == ctr_data.NULL_KEY, text[:, :13] == "")
    assert np.array_equal(keys[:, 13:] == ctr_data.EMPTY_KEY, text[:, 13:] == "")
    assert (text[:, :13] == "").any() and (text[:, 13:] == "").any(), "the sample lost its empty fields"
    # spot values of convert_numeric_feature and of the hexadecimal fields, straight from the text
    import math

    for r, c in ((0, 0), (3, 5), (17, 12), (99, 1)):
        if text[r, c] != "":
            v = int(text[r, c])
            assert keys[r, c] == (int(math.log(v) ** 2) if v > 2 else v - 2)
    for r, c in ((0, 13), (50, 20), (99, 38)):
        if text[r, c] != "":
            assert keys[r, c] == int(text[r, c], 16)


def test_reader_skips_other_column_counts_and_keeps_line_numbers(tmp_path):
    with open(ch.SAMPLE) as f:
        lines = f.readlines()
    path = tmp_path / "holes.txt"
    path.write_text(lines[0] + "1\t2\t3\n" + lines[1] + "\n" + lines[2])
    keys, labels, line_no = pkg.read_criteo_text(str(path))
    assert line_no.tolist() == [0, 2, 4] and keys.shape == (3, 39)
    assert np.array_equal(keys, pkg.read_criteo_text(ch.SAMPLE)[0][:3])


@pytest.mark.parametrize("threshold", ch.THRESHOLDS)
def test_restated_rule_against_the_reference_mapper(sample, golden, threshold):
    keys, labels, _ = sample
    records, dims = ch.encode_restated(keys, labels, threshold)
    rows, want_dims, defaults = golden[f"rows_t{threshold}"], golden[f"field_dims_t{threshold}"], golden[f"defaults_t{threshold}"]
    assert np.array_equal(dims, want_dims.astype(np.int64))
    assert int(dims.sum()) == ch.SUM_DIMS[threshold]
    assert np.array_equal(records[:, 0], rows[:, 0])
    ours_oov = records[:, 1:] == (dims - 1)
    assert np.array_equal(ours_oov, rows[:, 1:] == defaults)
    for f in range(39):
        pairs = {(int(a), int(b)) for a, b in zip(records[:, 1 + f], rows[:, 1 + f])}
        assert len({a for a, _ in pairs}) == len(pairs) == len({b for _, b in pairs}), f"field {f}: no bijection"


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 1000, 4096, 4097])
def test_restated_p_is_a_permutation(n):
    for seed, epoch in ((0, 0), (1234567, 3)):
        p = ch.p_restated(np.arange(n), n, seed, epoch)
        assert np.array_equal(np.sort(p), np.arange(n))
        some = sorted({0, n // 2, n - 1})
        assert [ch.p_scalar(j, n, seed, epoch) for j in some] == p[some].tolist()


def test_sixty_four_epochs_give_sixty_four_orders():
    orders = {ch.p_restated(np.arange(4096), 4096, 7, e).tobytes() for e in range(64)}
    assert len(orders) == 64


def test_argument_errors_that_need_no_device():
    records = np.zeros((5, 4), dtype=np.uint32)
    with pytest.raises(ValueError, match="field_dims"):
        pkg.DeviceCTRDataset(records, [2, 2])
    with pytest.raises(ValueError, match="index"):
        pkg.DeviceCTRDataset(records, [2, 2, 2], index=torch.tensor([0, 5]))
    with pytest.raises(ValueError, match="index"):
        pkg.DeviceCTRDataset(records, [2, 2, 2], index=np.array([-1, 0]))
    with pytest.raises(ValueError, match="batch_size"):
        pkg.DeviceCTRLoader(object(), 0)
    with pytest.raises(ValueError, match="min_threshold"):
        pkg.encode_ctr_columns(np.zeros((2, 2), dtype=np.int64), np.zeros(2, dtype=np.uint8), 0)
