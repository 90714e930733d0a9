"""Host tier of the central-difference Jacobians (csrc/lsq_fd.hip, api.py): the step constant, the coloured host twin against
the dense twin, and the refusal that stays.  No GPU.

The models are polynomials in + and * only: numpy evaluates them elementwise with correctly rounded operations, so a row's
value cannot depend on its position in the vector or on what the other blocks' entries hold -- the coloured twin (column c of
every block perturbed at once) and the dense twin (one column at a time) must then agree bit for bit."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import lsq_amd as lsq
from lsq_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eps3_literal():
    eps3 = np.finfo(float).eps ** (1.0 / 3.0)
    assert float.fromhex("0x1.965fea53d6e41p-18") == eps3
    assert api.FD_EPS3 == eps3
    assert float(np.cbrt(np.finfo(float).eps)) != eps3         # (the neighbouring double: ...e3d)
    src = open(os.path.join(ROOT, "leastsquaresoptim.jl_amd", "csrc", "lsq_fd.hip")).read()
    lit = re.findall(r"FD_EPS3\s*=\s*(0x[0-9a-fA-F.]+p[-+]?\d+)", src)
    assert lit == ["0x1.965fea53d6e41p-18"], lit
    assert "0x1.965fea53d6e41p-18" in open(os.path.join(ROOT, "include", "lsqhip.h")).read()


def test_symbol_declared_and_bound():
    import julia_shim_lint as JL
    assert "lsq_fd_jacobian" in lsq.declared_symbols()
    ret, params = JL.header_prototypes()["lsq_fd_jacobian"]
    assert ret == "int" and params == ["ptr:void", "ptr:void", "ptr:double", "ptr:void", "ptr:void"]
    hdr = open(os.path.join(ROOT, "include", "lsqhip.h")).read()
    assert "types.jl:54-58" in hdr


def special_x(n, seed):
    """Every kind of entry the step rule distinguishes: +-0, negative, |x| large (relative step), tiny (absolute step)."""
    x = np.random.default_rng(seed).uniform(-2.0, 2.0, n)
    for k, v in enumerate((0.0, -0.0, -3.5, 1e8, 1e-300, -1e8)):
        if k < n:
            x[(k * 7) % n] = v
    return x


def poly_model(B, mb, nb, ng, seed):
    """r_{b,i} = sum_c a_{b,i,c} x_{b,c} (1 + x_{b,c}) + sum_k w_{b,i,k} (g_k + g_k g_k) + x_{b,0} g_0 (if ng): + and * only."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((B, mb, nb))
    w = rng.standard_normal((B, mb, max(ng, 1)))

    def f_(out, x):
        xl = x[:B * nb].reshape(B, nb)
        acc = np.zeros((B, mb))
        for c in range(nb):
            xc = xl[:, c][:, None]
            acc = acc + a[:, :, c] * (xc * (1.0 + xc))
        for k in range(ng):
            gk = x[B * nb + k]
            acc = acc + w[:, :, k] * (gk + gk * gk)
        if ng:
            acc = acc + xl[:, 0][:, None] * x[B * nb]
        out[:] = acc.reshape(-1)

    return f_


@pytest.mark.parametrize("shape", [(1, 1, 1, 0), (5, 3, 3, 0), (7, 4, 2, 0), (1, 2, 1, 1), (5, 7, 3, 2), (4, 6, 2, 3)])
def test_coloured_twin_equals_dense_twin(shape):
    B, mb, nb, ng = shape
    m, n = B * mb, B * nb + ng
    f_ = poly_model(B, mb, nb, ng, 11)
    x = special_x(n, 5)
    J = lsq.BorderedBlockDiagonal(B, mb, nb, ng) if ng else lsq.BlockDiagonal(B, mb, nb)
    J.data[:] = np.nan
    calls = [0]

    def counted(out, xx):
        calls[0] += 1
        f_(out, xx)

    api._colored_difference_jacobian(counted, m)(J, x)
    assert calls[0] == 2 * (nb + ng)                      # whatever B is
    D = np.full((m, n), np.nan, order="F")
    api._central_difference_jacobian(f_, m)(D, x)
    assert np.all(np.isfinite(J.data))
    S = J.toarray()
    mask = np.zeros((m, n), dtype=bool)
    for b in range(B):
        mask[b * mb:(b + 1) * mb, b * nb:(b + 1) * nb] = True
    mask[:, B * nb:] = True
    assert np.array_equal(S[mask], D[mask])               # bit for bit
    assert np.all(D[~mask] == 0.0)                        # outside the structure the dense twin finds exactly 0
    assert np.array_equal(S, np.where(mask, D, 0.0))


def test_default_g_on_block_handles_is_the_coloured_twin():
    B, mb, nb, ng = 3, 4, 2, 1
    for J in (lsq.BlockDiagonal(B, mb, nb), lsq.BorderedBlockDiagonal(B, mb, nb, ng)):
        g = getattr(J, "ng", 0)
        f_ = poly_model(B, mb, nb, g, 3)
        x = special_x(B * nb + g, 9)
        nls = lsq.LeastSquaresProblem(x=x, y=np.zeros(B * mb), f_=f_, J=J)
        assert api._device_fd(nls)
        nls.g_(nls.J, nls.x)
        ref = type(J)(*((B, mb, nb, g) if g else (B, mb, nb)))
        api._colored_difference_jacobian(f_, B * mb)(ref, x)
        assert np.array_equal(nls.J.data, ref.data)
        nls.g_ = lambda Jm, xx: None                      # a g_ of the user's own ends the default
        assert not api._device_fd(nls)
    # the dense default stays the host twin
    nls = lsq.LeastSquaresProblem(x=np.ones(2), y=np.zeros(3), f_=lambda out, xx: None)
    assert not api._device_fd(nls)


def test_csc_without_g_still_raises():
    S = sp.csc_matrix(np.eye(3))
    nls = lsq.LeastSquaresProblem(x=np.ones(3), y=np.zeros(3), f_=lambda out, x: out.__setitem__(slice(None), x * x), J=S)
    assert not api._device_fd(nls)
    with pytest.raises(lsq.ArgumentError):
        nls.g_(nls.J, nls.x)
