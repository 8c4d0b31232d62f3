"""The exact one-soliton solution of the Korteweg-de Vries equation

    u_t + a1 u u_x + d3 u_xxx = 0:      u(x, t) = (3 c / a1) sech^2( 1/2 sqrt(c / d3) (x - c t - x_0) ),

a closed form, so there is neither a solver nor a data file.  With the defaults (a1 = 1, d3 = 0.0025, c = 0.5, x_0 = -0.3) the
wave crosses x in [-1, 1] from -0.2 at t = 0.2 to 0.1 at t = 0.8 and stays below 1e-4 at both walls in between.

In the engine's coefficient order (a0, a1, nu, r1, r2, r3, d3) the truth is KDV_COEFFS: no diffusion, nu = 0.
"""
import numpy as np

A1, D3, C, X0 = 1.0, 0.0025, 0.5, -0.3
LB, UB = -1.0, 1.0
KDV_COEFFS = (0.0, A1, 0.0, 0.0, 0.0, 0.0, D3)


def soliton(x, t, a1=A1, d3=D3, c=C, x0=X0):
    """u(x, t); x and t broadcast"""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    return (3.0 * c / a1) / np.cosh(0.5 * np.sqrt(c / d3) * (x - c * t - x0)) ** 2


def snapshot(t, n=512, lb=LB, ub=UB, **kw):
    """-> x [n, 1] (uniform grid, both walls included), u(x, t) [n, 1]"""
    x = np.linspace(lb, ub, n)[:, None]
    return x, soliton(x, t, **kw)
