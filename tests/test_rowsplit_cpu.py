"""recbole_amd/csrc/rowsplit.h against the four row-split rules it replaced, on the host.

The weight gradients of K16c (NGCF), K18c (CIN), K19b (cross network) and K20b (AFM) are sums
of per-split partials in split order, so their bits rest on (rows, splits) as a function of
the row count. tools/check_rowsplit.cpp includes only the header, is built with the host C++
compiler and prints row_split's answer for every tuple on its stdin; each must equal the
kernel's own rule as it stood before the header, restated here one kernel at a time. Nothing
is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which(os.environ.get('CXX') or 'c++') or shutil.which('g++') or shutil.which('clang++')


def _ceil(a, b):
    return (a + b - 1) // b


# ---- the four rules as each kernel's host code wrote them: R rows -> (rows, splits)
def ngcf_rule(n):
    rows = _ceil(n, 512)
    rows = (rows + 15) // 16 * 16
    rows = max(rows, 256)
    return rows, _ceil(n, rows)


def cin_want(m, H):
    units = H * ((m + 15) // 16) + 1
    groups = (units + 4 - 1) // 4                 # four waves a workgroup
    return min(32, max(1, 512 // groups))


def cin_rule(R, m, H):
    want = cin_want(m, H)
    r = _ceil(R, want)
    r = max((r + 32 - 1) // 32 * 32, 256)
    return r, _ceil(R, r)


def cross_rule(B):
    r = _ceil(B, 32)
    r = max((r + 8 - 1) // 8 * 8, 8)
    return r, _ceil(B, r)


def afm_rule(B):
    r = max(_ceil(B, 32), 1)
    return r, _ceil(B, r)


# ---- what each kernel now hands row_split: (most, multiple, least)
NGCF = (512, 16, 256)
CROSS = (32, 8, 8)
AFM = (32, 1, 1)


def cin_params(m, H):
    return (cin_want(m, H), 32, 256)


ROWS = sorted(set(range(1, 5000)) |
              {(1 << k) + d for k in range(35) for d in (-1, 0, 1) if (1 << k) + d >= 1})
CIN_SHAPES = [(m, H) for m in (2, 16, 17, 39, 64) for H in (1, 39, 100, 256)]

# the values the GPU tests assert through the library
PINNED = [(AFM, 2065, (65, 32)), (NGCF, 5200, (256, 21)), (NGCF, 190, (256, 1)),
          (CROSS, 2048, (64, 32)), (CROSS, 2065, (72, 29))]


@pytest.mark.skipif(CXX is None, reason='no C++ compiler on this machine')
def test_row_split_reproduces_the_four_rules(tmp_path):
    exe = str(tmp_path / 'check_rowsplit')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall',
                    os.path.join(ROOT, 'tools', 'check_rowsplit.cpp'), '-o', exe], check=True)
    cases = []                                    # (tuple for the program, expected, label)
    for params, R, want in PINNED:
        cases.append(((R,) + params, want, ('pinned', R)))
    for R in ROWS:
        cases.append(((R,) + NGCF, ngcf_rule(R), ('ngcf', R)))
        cases.append(((R,) + CROSS, cross_rule(R), ('cross', R)))
        cases.append(((R,) + AFM, afm_rule(R), ('afm', R)))
        for m, H in CIN_SHAPES:
            cases.append(((R,) + cin_params(m, H), cin_rule(R, m, H), ('cin', R, m, H)))
    text = ''.join('%d %d %d %d\n' % c[0] for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout
    got = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    assert len(got) == len(cases)
    bad = [(c[2], g, c[1]) for c, g in zip(cases, got) if g != c[1]]
    assert not bad, bad[:10]
    # the rules' own promises: no more splits than `most`, and the last split is not empty
    for (R, most, _, _), (rows, splits) in zip((c[0] for c in cases), got):
        assert 1 <= splits <= most and (splits - 1) * rows < R <= splits * rows
    # the CIN's `most` at the ends of its range: one unit group takes 32 splits, the widest
    # layer one
    assert cin_want(2, 1) == 32 and cin_want(39, 100) == 6 and cin_want(64, 256) == 1
