"""CPU certificate of the window-edge inputs of tests/test_gpu_text.py (parse_kernel's windows:
1 KB at DSM_PARSE_BPL=16, 2 KB at the default 32; a file's windows start at its offset in the
concatenated text rounded down to 16).

Of the 125 (line kind, interior byte offset) pairs of the 15 well-formed LINES, the files built
when 1 KB was the only window size put 78 on a 1 KB window boundary and 31 on a 2 KB one; with the
constructed files all 125 are on one at both sizes.  The host reader (the expected values of the
GPU test) reads every constructed file to its last line at 8 nodes."""
import pytest

import test_gpu_text as T


@pytest.fixture(scope="module")
def inputs():
    return T._window_edge_files()


def test_every_pair_on_a_window_boundary(inputs):
    files, first = inputs
    pairs = {(k, o) for k in range(15) for o in range(1, len(T.LINES[k]))}
    assert len(pairs) == 125
    old = {win: len(T.window_pairs_covered(files[:first], win)) for win in T.WINDOWS}
    print("covered by the earlier files alone:", old)
    assert old == {1024: 78, 2048: 31}
    for win in T.WINDOWS:
        assert T.window_pairs_covered(files, win) == pairs
    # ... and on a 16-byte lane boundary (a window boundary is one)
    assert T.window_pairs_covered(files, 16) == pairs


def test_constructed_files_meet_their_boundary(inputs):
    """Each constructed file crosses into its second window (or ends at it, or one byte past)."""
    files, first = inputs
    b0 = sum(len(f) for f in files[:first])
    n_pairs = 125
    per_win = n_pairs + 4 + 19 + 3 * (1 + 1 + 2)
    assert len(files) - first == 2 * per_win
    for i, data in enumerate(files[first:]):
        win = T.WINDOWS[i // per_win]
        end = b0 + len(data) - (b0 & ~15)
        assert win <= end < win + 64, (i, win, end)
        b0 += len(data)


def test_host_reader_reads_constructed_files_to_the_end(inputs, tmp_path):
    import pydsm
    files, first = inputs
    exp = T._host_expect(pydsm, tmp_path, files[first:], 8, 512)
    for data, (n, rc, _) in zip(files[first:], exp):
        want = sum(-(-len(ln) // 19) for ln in data.splitlines(keepends=True))
        assert (n, rc) == (want, 0), data[-80:]
    # at 4 nodes only the files built around "RD 0x7f" (home 7) and "WR 0x45 -1" (home 4) end
    # early, at that line on the window boundary
    exp4 = T._host_expect(pydsm, tmp_path, files[first:], 4, 512)
    bad = [i for i, (_, rc, _) in enumerate(exp4) if rc != 0]
    assert len(bad) == 2 * (len(T.LINES[5]) - 1 + len(T.LINES[6]) - 1)
    assert all(exp4[i][1] == pydsm.E_RANGE and exp4[i][0] == exp[i][0] - 3 for i in bad)
