"""recbole_amd/csrc/drop.h against its numpy restatement (tests/drop_spec.py), on the host:
tools/check_drop.cpp includes only that header, is built with the host C++ compiler and
prints the key, the thresholds and the keep bits of elements 0..4095 (from drop_keep and
from drop_keep4); every figure must equal the specification's exactly. Nothing is loaded
into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import drop_spec as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which(os.environ.get('CXX') or 'c++') or shutil.which('g++') or shutil.which('clang++')

SEED, COUNTER, P = ds.ln_site_seed(2020, ds.ln_ffn(1)), 7, 0.3
THRESHOLD_PS = (1e-9, 0.1, 0.5, 0.9, 1.0 - 2.0 ** -24)


@pytest.mark.skipif(CXX is None, reason='no C++ compiler on this machine')
def test_drop_header_matches_spec(tmp_path):
    exe = str(tmp_path / 'check_drop')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', os.path.join(ROOT, 'tools', 'check_drop.cpp'),
                    '-o', exe], check=True)
    out = subprocess.run([exe, str(SEED), str(COUNTER), repr(P)], check=True,
                         capture_output=True, text=True).stdout.split('\n')
    assert out[0] == f'key {int(ds.key(SEED, COUNTER))}'
    thr = [line.split() for line in out[1:6]]
    assert [t[0] for t in thr] == ['thr'] * 5
    assert [float(t[1]) for t in thr] == list(THRESHOLD_PS)     # the program's own p list
    assert [int(t[2]) for t in thr] == [ds.threshold(p) for p in THRESHOLD_PS]
    assert ds.threshold(THRESHOLD_PS[0]) < 4294967295 and ds.threshold(THRESHOLD_PS[-1]) == 256
    want = ds.ln_keep(SEED, COUNTER, 4096, P)
    assert 0 < int(want.sum()) < 4096
    for line, name in ((out[6], 'keep'), (out[7], 'keep4')):
        head, bits = line.split()
        assert head == name and len(bits) == 4096
        assert np.array_equal(np.frombuffer(bits.encode(), dtype=np.uint8) == ord('1'), want)
