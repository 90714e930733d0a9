"""Handle state tier, CPU certification (tests/handle_state_common.py; the device part is tests/test_t_gpu_handle_state.py).

  1. The twin: its effective matrix and every reader's reference against scipy / numpy in plain fp64, after mutations of
     every kind -- oracle 2 accepts a correct fp64 evaluation.
  2. Coverage of the committed sequences, per configuration: every ordered (mutation, reader) pair and every ordered
     (mutation, mutation) pair that some state allows occurs.  A condition on the seeds, not a measurement.
  3. Planted staleness: for every (mutation, reader) pair of the committed sequences, a reader that still sees the values from
     BEFORE the mutation is rejected by oracle 2 at more than 10 x its bound -- no committed mutation is a near no-op for any
     reader.  Exempt, because the reader's answer must not change there: mutations that change nothing (set_colscale(None)
     without a scale, the refused fd_jacobian_), values() under a mutation of the scale alone (it returns V), and the
     covariance of the plain CSC configurations, which is the documented LSQ_ENOTPD at their empty column whatever the values."""
import numpy as np
import pytest
import scipy.sparse as sp

import handle_state_common as H
from oracle import oracle as O

NAMES = list(H.CONFIGS)
SCALE_ONLY = ("set_colscale", "set_colscale_again", "s_inplace", "unscale")


def test_common_module_needs_no_device():
    import sys
    assert "torch" not in vars(H) and not any(getattr(v, "__name__", "") == "torch" for v in vars(H).values())
    assert "handle_state_common" in sys.modules


@pytest.mark.parametrize("name", NAMES)
def test_pattern_has_its_holes_and_the_committed_shape(name):
    cfg = H.CONFIGS[name]
    P = cfg.pattern
    assert P.shape == cfg.shape and P.has_sorted_indices
    if cfg.kind == "csc":
        rows, cols = np.diff(P.tocsr().indptr), np.diff(P.indptr)
        empty = slice(256, 512) if name == "small" else slice(3, 4)     # (test_m's pattern empties a whole gather window)
        assert np.all(rows[empty] == 0) and cols[1] == 0 and rows[5] == P.shape[1] - 1
    if name in ("sliced", "rows-only"):
        assert P.nnz >= 1 << 20             # the sliced layouts are built from 2^20 stored entries on
    if name == "windowed":
        assert P.nnz < 1 << 20 and P.shape[0] > 131072
    if name == "segments":
        assert P.shape[0] > 2048 and P.nnz < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_twin_against_scipy(name):
    cfg = H.CONFIGS[name]
    twin = H.Twin(cfg, 1)
    rng = np.random.default_rng(5)
    todo = ["g", "set_values", "unscale", "g"] if cfg.model and cfg.fused else ["g", "set_values"] if cfg.model else \
        ["set_values", "set_colscale", "s_inplace", "write_refresh", "set_colscale_again", "unscale", "async_wait"]
    for mu in todo:
        before = twin.eff64().copy()
        twin.mutate(mu, rng)
        E = twin.scipy()
        ratio = twin.eff64() / before
        assert np.all(((ratio >= 0.4999) & (ratio <= 0.8001)) | ((ratio >= 1.2499) & (ratio <= 2.0001))), (mu, ratio.min(), ratio.max())
        dense = sp.csc_matrix((twin.V, twin.indices, twin.indptr), shape=cfg.shape)
        if twin.s is not None:
            dense = dense @ sp.diags(twin.s)
        assert abs(E - dense).max() <= 4e-16 * abs(E).max()
        for reader in cfg.readers:
            q = H.judge(twin, reader, H.host_read(twin, reader, O), O)
            assert q <= 1.0, (mu, reader, q)


@pytest.mark.parametrize("name", NAMES)
def test_committed_sequences_cover_every_pair(name):
    cfg = H.CONFIGS[name]
    seqs = H.sequences(cfg)
    assert len(seqs) == H.NSEQ[name] and all(len(s) == H.SEQ_LEN for s in seqs)
    assert seqs == H.sequences(cfg)                                   # fixed seeds: the same walk every time
    mm, mr = H.coverage(cfg, seqs)
    assert {(a, r) for a in cfg.mutations for r in cfg.readers} <= mr
    assert H.legal_pairs(cfg) <= mm, sorted(H.legal_pairs(cfg) - mm)
    for steps in seqs:
        assert set(steps[-1][1]) == set(cfg.readers) and all(len(rs) == 2 for _, rs in steps[:-1])
        scaled = cfg.model and cfg.fused
        for mu, _ in steps:
            assert cfg.legal(mu, scaled), (mu, scaled)
            scaled = cfg.after(mu, scaled)


def exempt(cfg, twin, mu, reader):
    if mu in ("unscale_plain", "fd_refused"):
        return True
    if reader == "values" and (mu in SCALE_ONLY or (mu == "g" and cfg.fused)):
        return True
    return reader in ("cov", "cov_qr") and twin.empty_col is not None


@pytest.mark.parametrize("name", NAMES)
def test_planted_staleness_is_rejected(name):
    cfg = H.CONFIGS[name]
    done = set()
    for k, steps in enumerate(H.sequences(cfg)):
        twin = H.Twin(cfg, H._seed(cfg, k))
        for i, (mu, readers) in enumerate(steps):
            before = twin.copy()
            twin.mutate(mu, H.step_rng(cfg, k, i))
            for reader in readers:
                if (mu, reader) in done or exempt(cfg, twin, mu, reader):
                    continue
                done.add((mu, reader))
                q = H.judge(twin, reader, H.host_read(before, reader, O), O)
                assert q > 10.0, (name, k, i, mu, reader, q)
    want = {(a, r) for a in cfg.mutations for r in cfg.readers if not exempt(cfg, H.Twin(cfg, 0), a, r)}
    assert want <= done, sorted(want - done)
