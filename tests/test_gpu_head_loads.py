"""The sweep kernels request their model values and first data in one group at the top, ahead of the guards that used to
stand in front of those loads.  What can go wrong with that shows on the smallest grids - a single block, a chunk that ends
one block past a boundary - so: chains whose every position is a block (weights scaled by 1e9), at lengths on both sides of a
forward chunk (4 blocks), a backward chunk (64) and a reduction chunk (256), for 2, 5 and 10 states (from 8 states on the
transition matrix lives in LDS), against the device-mode checker, bit for bit."""
import re

import numpy as np
import pytest

from tests.test_gpu_parity import bits, compare_state, make_pair, run_both, setup_model

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 5, 63, 64, 65, 255, 256, 257, 1025]
SCHEME = [("F", 6, 1)]


def set_up(o, g, x, K):
    """The automatic prior, as everywhere - except for a single observation: its data variance is zero, which the prior's
    rule refuses (checker and library alike), so both sides are given one fixed prior instead."""
    if len(x) > 1:
        return setup_model(o, g, K)
    p = np.array([2.0, 0.1, float(x[0]), 1.0], np.float32)
    o.set_prior(p)
    o.init_model()
    g.set_model(K, p, 0.5, 0.5, 0.5, True)
    return p


def run_chain(hml, T, K, weight_keys=None):
    x, o, g = make_pair(hml, T, K, 7, 42, weight_keys=weight_keys, weight_mult=1e9)
    set_up(o, g, x, K)
    g._pending_prior = True
    o.set_record(marginals=True)
    run_both(o, g, SCHEME)
    return o, g


@pytest.mark.parametrize("K", [2, 5, 10])
@pytest.mark.parametrize("T", LENGTHS)
def test_every_position_a_block(hml, T, K):
    o, g = run_chain(hml, T, K)
    assert len(g.blocks()) == T + 1, "every position a block"   # (the starts and the end marker)
    compare_state(o, g, what="T = %d, %d states" % (T, K))       # blocks, states, theta, A, pi
    seg, cnt = g.marginals_rle()
    assert hml.marginals_text(seg, cnt) == o.text("marginals")


@pytest.mark.parametrize("K", [5, 10])
@pytest.mark.parametrize("T", LENGTHS)
def test_every_position_a_block_through_the_fused_block_kernel(hml, T, K):
    """The same chains with option weight_keys = 2: the block structure comes from the fused block kernel in EVERY sweep (by
    default a chain this weakly compressed leaves it after the first) - its summary words are requested ahead of their guards
    on a grid of one tile, with fewer starts than threads and (T = 1025) more; 10 states take the looped emission terms."""
    o, g = run_chain(hml, T, K, weight_keys=2)
    assert len(g.blocks()) == T + 1, "every position a block"
    assert g.stats()["fused_fallbacks"] == 0
    compare_state(o, g, what="T = %d, %d states, fused block kernel" % (T, K))
    seg, cnt = g.marginals_rle()
    assert hml.marginals_text(seg, cnt) == o.text("marginals")


def test_stage_stamps_do_not_change_the_chain(hml, monkeypatch, capfd):
    """HML_PARAMS_DEBUG=1 makes the parameter kernel stamp its stages (the flag travels with the model; the stamps are
    printed when the chain is synchronised); the chain is the one it is without the stamps."""
    T, K = 1025, 5
    o, plain = run_chain(hml, T, K)
    assert "[params dbg]" not in capfd.readouterr().err
    monkeypatch.setenv("HML_PARAMS_DEBUG", "1")
    o2, stamped = run_chain(hml, T, K)
    # the flag reached the kernel: stamps that lie behind the kernel's start
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[params dbg] us since")]
    assert lines, "no stage stamps were printed"
    end = [float(v) for v in re.findall(r"end ([0-9.]+)", lines[-1])]
    assert end and 0.0 < end[0] < 1e4, lines[-1]
    compare_state(o2, stamped, what="with stage stamps")
    assert np.array_equal(plain.blocks(), stamped.blocks())
    assert np.array_equal(plain.states(), stamped.states())
    assert np.array_equal(bits(plain.theta()), bits(stamped.theta()))
    Ap, pp = plain.transitions()
    As, ps = stamped.transitions()
    assert np.array_equal(bits(Ap), bits(As)) and np.array_equal(bits(pp), bits(ps))
    text = hml.marginals_text(*stamped.marginals_rle())
    assert text == hml.marginals_text(*plain.marginals_rle())
    assert text == o2.text("marginals")
