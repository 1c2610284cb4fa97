"""The float-free model of CTC decoding (tests/ctc_decode_reference.py) against hand-worked cases and an independent full-table
Levenshtein distance.  No GPU."""
import numpy as np

from ctc_decode_reference import argmax_rows, best_path, decode_fraction, levenshtein

A, B, BLANK = 0, 1, 2


def one_hot(path, C=3):
    y = np.full((len(path), C), 0.1, np.float32)
    y[np.arange(len(path)), path] = 0.8
    return y


def test_repeat_across_a_blank_is_kept():
    """a a _ a b b _  ->  a a b"""
    assert best_path(one_hot([A, A, BLANK, A, B, B, BLANK]), 7, BLANK) == [A, A, B]
    assert best_path(one_hot([A, A, BLANK, A, B, B, BLANK]), 3, BLANK) == [A]           # the frames behind `length` take no part
    assert best_path(one_hot([A, BLANK, A]), 3, BLANK) == [A, A]
    assert best_path(one_hot([B]), 1, BLANK) == [B] and best_path(one_hot([B]), 0, BLANK) == []


def test_all_blanks_decode_to_nothing():
    assert best_path(one_hot([BLANK] * 5), 5, BLANK) == []


def test_a_tie_picks_the_lowest_index():
    y = np.array([[0.2, 0.4, 0.4], [0.5, 0.0, 0.5], [0.0, 0.0, 0.0], [0.1, 0.3, 0.6]], np.float32)
    assert list(argmax_rows(y)) == [1, 0, 0, 2]
    assert np.array_equal(argmax_rows(y), np.argmax(y, axis=-1))
    assert best_path(y, 4, BLANK) == [B, A]            # b, a, a, blank
    rng = np.random.RandomState(0)
    z = rng.randint(0, 4, (50, 7, 9)).astype(np.float32)           # many ties
    assert np.array_equal(argmax_rows(z), np.argmax(z, axis=-1))


def test_distances_against_empty():
    assert levenshtein([], []) == 0
    assert levenshtein([], [1, 2, 3]) == 3 and levenshtein([4, 4], []) == 2
    assert levenshtein([1, 2, 3], [1, 2, 3]) == 0
    assert levenshtein([1, 2, 3], [1, 3]) == 1 and levenshtein([1, 2, 3], [1, 4, 3]) == 1 and levenshtein([1, 3], [3, 1]) == 2
    assert levenshtein("kitten", "sitting") == 3


def full_table(a, b):
    d = np.zeros((len(a) + 1, len(b) + 1), np.int64)
    d[:, 0] = np.arange(len(a) + 1)
    d[0, :] = np.arange(len(b) + 1)
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i, j] = min(d[i - 1, j] + 1, d[i, j - 1] + 1, d[i - 1, j - 1] + (a[i - 1] != b[j - 1]))
    return int(d[len(a), len(b)])


def test_levenshtein_against_the_full_table():
    rng = np.random.RandomState(1)
    for _ in range(200):
        a = list(rng.randint(0, 4, rng.randint(0, 25)))
        b = list(rng.randint(0, 4, rng.randint(0, 25)))
        assert levenshtein(a, b) == full_table(a, b) == levenshtein(b, a)


def test_decode_fraction():
    y = np.stack([one_hot([A, A, BLANK, A, B]), one_hot([B, B, B, A, A]), one_hot([A, B, A, B, A])], axis=1)
    pat = np.array([[1, 1, 0], [2, 2, 0], [2, 3, 0], [2, 0, 0], [3, 0, 0]], np.int8)
    k, decoded, dist = decode_fraction(y, pat, [[A, B], [B], []])
    assert decoded == [[A, A, B], [B], []] and list(dist) == [1, 0, 0]
    assert k[3, 1] == -1 and not (k[:, 2] != -1).any() and list(k[:, 0]) == [A, A, BLANK, A, B]
    assert decode_fraction(y, pat, None)[2] is None
