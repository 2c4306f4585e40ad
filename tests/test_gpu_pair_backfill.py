"""Option "side_order" 2: the merged launch of the --temporal step's forked passes (march_pair_kernel) picks its arrangement
on the device from the number of live samples -- A (the one of "side_order" 0) when one resident round of wave slots holds
the live tasks of both sub-passes, B (the student's tasks first, the ensemble pass behind them in 8-row segments) otherwise.

The gate is the one of tests/test_gpu_aug_skip.py: the step EQUALS the step under "student_overlap" 1 (a launch per pass, every
sample computed) under == in every loss scalar and leaf gradient, with the step workspace filled with NaN beforehand -- eagerly,
and from ONE captured graph whose augmentation tensor is rewritten between replays so that the live count crosses the A/B
threshold in both directions.  Option "device_cus" shrinks the round (8 slots per CU) so that tiny shapes reach B; which
arrangement each pattern takes is asserted from the restated arithmetic (tests/pair_backfill_checks.py)."""
import collections

import pytest
import torch

from mal_amd.synthetic import make_batch
from tests import pair_backfill_checks as P
from tests.test_gpu_aug_skip import SEED, Runner, _batch, _equal, _get, _lib, _run, _set, check_against_the_oracle

pytestmark = pytest.mark.gpu
OPTIONS = ("student_overlap", "side_order", "march_rows", "march_rows_fwd", "device_cus")


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


@pytest.fixture(autouse=True)
def _restore():
    """the options and the noise source as they were, failures included"""
    from mal_amd import config
    saved = {k: _get(k) for k in OPTIONS}
    noise = config.noise_source, config.noise_seed
    config.noise_source, config.noise_seed = "philox", SEED
    try:
        yield
    finally:
        config.noise_source, config.noise_seed = noise
        for k, v in saved.items():
            _lib().mal_set_option(k.encode(), v)


Case = collections.namedtuple("Case", "name B H W no_ens cus rows rows_fwd patterns takes why")
# patterns: augmentation masks in the order they are run and replayed; takes: the arrangement of each ("-": no merged launch)
CASES = [
    Case("b2_40x130", 2, 40, 130, False, 1, 0, 0, [(0, 0), (1, 0), (0, 0), (1, 1), (0, 1)], "BABAA",
         "the smallest: 6 + 6 tasks against 8 slots, the short ensemble pass has 5 segments"),
    Case("b3_37x50", 3, 37, 50, False, 1, 0, 0, [(0, 0, 0), (1, 0, 0), (0, 0, 0), (0, 1, 1)], "BABA",
         "ragged last short segment (37 = 4 * 8 + 5); two live samples sit ON the threshold (8 tasks, 8 slots)"),
    Case("b1_16x61", 1, 16, 61, False, 1, 0, 0, [(0,), (1,), (0,)], "AAA",
         "4 + 2 tasks: the short decomposition is the long one, the grid's surplus is empty"),
    Case("b9_24x122", 9, 24, 122, False, 2, 8, 24, [(1,) * d + (0,) * (9 - d) for d in (0, 8, 1, 9, 0)], "BABAB",
         "0, 1, 8, 9 dead; 9 + 2 tasks per sample against 16 slots; short ensemble 3 segments against 1"),
    Case("b2_40x130_no_ens", 2, 40, 130, True, 1, 8, 0, [(0, 0), (1, 1), (1, 0), (0, 1)], "BABB",
         "--no_ens: no ensemble workgroups at all; 15 student tasks per sample against 8 slots"),
    Case("b65_16x24", 65, 16, 24, False, 1, 16, 16, [(0,) * 65, (1, 0) * 32 + (1,), (1,) * 64 + (0,)], "---",
         "outside march_pair_qualifies: a launch per pass, ordered as under 0"),
]


def _options(c):
    _set(device_cus=c.cus, march_rows=c.rows, march_rows_fwd=c.rows_fwd)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_side_order_2_equals_no_skip(c):
    _options(c)
    if c.B <= 64:
        takes = "".join(P.arrangement_of(p, c.B, c.H, c.W, c.no_ens, c.rows, c.rows_fwd, c.cus) for p in c.patterns)
        assert takes == c.takes, takes
    kw = {"temporal": True, "no_ens": True} if c.no_ens else {"temporal": True}
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        r = Runner(_batch(c.B, c.H, c.W), kw)
        refs = [_run(r, 1, p) for p in c.patterns]
        for p, ref in zip(c.patterns, refs):
            _equal(_run(r, 2, p, side_order=2), ref, (c.name, "eager", p))
        # one graph, captured on THIS stream (the step's workspace is keyed by the stream) with the first pattern
        _set(student_overlap=2, side_order=2)
        r.set_pattern(c.patterns[0])
        r.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s_, capture_error_mode="thread_local"):
            r.step()
        for p, ref in list(zip(c.patterns, refs))[1:] + [(c.patterns[0], refs[0])]:
            r.set_pattern(p)
            r.poison()
            for t in r.leaves.values():
                t.grad.zero_()
            graph.replay()
            _equal(r.result(), ref, (c.name, "replay", p))
    torch.cuda.current_stream().wait_stream(s_)


def test_against_the_oracle_in_arrangement_b():
    """B=12 at 24x122, samples 0 and 3..8 augmented (the batch of tests/test_gpu_aug_skip_sweep.py): five live samples,
    9 + 2 tasks each against 16 slots"""
    B, H, W = 12, 24, 122
    mask = (1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0)
    _set(device_cus=2, march_rows=8, march_rows_fwd=24, side_order=2)
    assert P.arrangement_of(mask, B, H, W, False, 8, 24, 2) == "B"
    b = make_batch(B, H, W, seed=323, with_syn=True)
    b["augmentation_mask"] = torch.tensor(mask, dtype=torch.float32).reshape(b["augmentation_mask"].shape)
    torch.manual_seed(1)
    n0, n1 = torch.randn(B, 1, H, W), torch.randn(B, 1, H, W)
    check_against_the_oracle(b, {"temporal": True}, n0, n1)


def test_option_range():
    lib = _lib()
    for v in (0, 1, 2):
        assert lib.mal_set_option(b"side_order", v) == 0 and _get("side_order") == v
    assert lib.mal_set_option(b"side_order", 3) == -1 and lib.mal_set_option(b"side_order", -1) == -1
    assert _get("side_order") == 2
