"""GPU: error behaviour of the C ABI (every misuse is a PINN_E* code with a message, never a crash): the reference
would raise from Keras / numpy shape checks at the same call sites."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LB, UB = np.array([-1.0, 0.0]), np.array([1.0, 0.99])


def test_misuse_raises_with_a_message():
    import pinn_native
    E = pinn_native.PinnNativeError
    eng = pinn_native.Engine([2, 20, 20, 1], LB, UB, pde="burgers", dtype="f32")
    with pytest.raises(E, match="not a discrete-time model"):
        eng.disc_set_stage(0, np.zeros(3), np.zeros(3), None)
    with pytest.raises(E, match="not a discrete-time model"):
        eng.disc_predict(0, np.zeros(3))
    with pytest.raises(E, match="Schrodinger-only"):
        eng.set_boundary(np.zeros((2, 2)), np.zeros((2, 2)))
        eng.set_collocation(np.zeros((4, 2)))
        eng.loss_grad()
    eng.close()
    eng = pinn_native.Engine([2, 20, 20, 1], LB, UB, pde="burgers_ide", dtype="f32")
    with pytest.raises(E, match="no collocation set"):
        eng.lhs_collocation(100, seed=1)
    with pytest.raises(E, match="mailboxes are not attached"):
        eng.comm_set_mode("mailbox")
    with pytest.raises(E):
        eng.set_weights(np.zeros(5))
    eng.close()
    with pytest.raises(E, match="hidden widths must be equal"):
        pinn_native.Engine([2, 20, 30, 1], LB, UB, pde="burgers")
    with pytest.raises(E, match="one input"):
        pinn_native.Engine([2, 20, 20, 5], LB, UB, pde="burgers_disc")
    with pytest.raises(E, match="output size"):
        pinn_native.Engine([2, 20, 20, 2], LB, UB, pde="burgers")
    d = pinn_native.Engine([1, 20, 20, 5], [-1.0], [1.0], pde="burgers_disc", dtype="f64")
    with pytest.raises(E, match="stage sets"):
        d.set_collocation(np.zeros((4, 2)))
    with pytest.raises(E, match="no stage set"):
        d.loss_grad()
    with pytest.raises(E, match="outside 1..n_out"):
        d.disc_set_stage(0, np.zeros(3), np.zeros(3), np.zeros((5, 9)))
    with pytest.raises(E, match="different q"):
        d.disc_set_stage(0, np.zeros(3), np.zeros(3), np.zeros((5, 4)))
        d.disc_set_stage(1, np.zeros(3), np.zeros(3), np.zeros((5, 3)))
        d.loss_grad()
    d.close()


# ---- the optional extras (self-adaptive weights, point weights, Robin points, a source term, coefficient fields): who
# ---- refuses whom, as whole sentences ----------------------------------------------------------------------------------
N_F, N_U, N_B, N_W = 64, 8, 2, 3
ADR_COEF = [0.0, 0.0, 1e-4, -5.0, 0.0, 5.0]
SETTERS = ("pinn_set_robin", "pinn_set_source", "pinn_set_coef_fields")
# the sentences, as the engine's source spells them.  An extra present -> pinn_comm_init and pinn_comm_xgmi_export say,
# behind their own name:
SINGLE_DEVICE = {
    "sa": "self-adaptive weights are single-device (pinn_sa_disable first)",
    "pw": "point weights are single-device (pinn_pw_disable first)",
    "robin": "Robin points are single-device (pinn_set_robin with n = 0 first)",
    "source": "a source term is single-device (pinn_set_source with n = 0 first)",
    "fields": "coefficient fields are single-device (pinn_set_coef_fields with n = 0 first)",
}
PATH_7_ONLY = {
    "sa": "pinn_set_kernel_path: self-adaptive weights run on kernel path 7 only (pinn_sa_disable first)",
    "pw": "pinn_set_kernel_path: point weights run on kernel path 7 only (pinn_pw_disable first)",
}
PW_SET = {
    "robin": "pinn_pw_set: point weights do not cover Robin points; remove them first (pinn_set_robin with n = 0)",
    "source": "pinn_pw_set: point weights are not combined with a source term; remove it first (pinn_set_source with n = 0)",
    "fields": "pinn_pw_set: point weights are not combined with coefficient fields; remove them first "
              "(pinn_set_coef_fields with n = 0)",
}
# the three setters, refused by point weights, on the adr_ide kind, on the kinds 0, 1 and 2, by a communicator
BY_POINT_WEIGHTS = {
    "pinn_set_robin": "pinn_set_robin: point weights do not cover Robin points (pinn_pw_disable first)",
    "pinn_set_source": "pinn_set_source: point weights are not combined with a source term (pinn_pw_disable first)",
    "pinn_set_coef_fields": "pinn_set_coef_fields: point weights are not combined with coefficient fields "
                            "(pinn_pw_disable first)",
}
ON_ADR_IDE = {
    "pinn_set_robin": "pinn_set_robin: Robin points are for the adr kind (pde 5) only; the adr_ide kind (pde 6) has no "
                      "variant for them",
    "pinn_set_source": "pinn_set_source: a source term is for the adr kind (pde 5) only; the adr_ide kind (pde 6) has no "
                       "variant for it",
    "pinn_set_coef_fields": "pinn_set_coef_fields: coefficient fields are for the adr kind (pde 5) only; the adr_ide kind "
                            "(pde 6) has no variant for them",
}
ON_OTHER_KINDS = {
    "pinn_set_robin": "pinn_set_robin: Robin points are for the adr kind (pde 5) only",
    "pinn_set_source": "pinn_set_source: a source term is for the adr kind (pde 5) only",
    "pinn_set_coef_fields": "pinn_set_coef_fields: coefficient fields are for the adr kind (pde 5) only",
}
BY_COMMUNICATOR = {
    "pinn_set_robin": "pinn_set_robin: Robin points are single-device; this context has a communicator",
    "pinn_set_source": "pinn_set_source: a source term is single-device; this context has a communicator",
    "pinn_set_coef_fields": "pinn_set_coef_fields: coefficient fields are single-device; this context has a communicator",
}


def _context(pde, dtype="f64"):
    """2-20-20-20-20-n_out (the smallest depth kernel path 7 takes), 64 collocation points, 8 data points and, where the kind
    has them, 2 boundary pairs: one or two tiles"""
    import pinn_native
    rs = np.random.RandomState(7)
    n_out = 2 if pde == "schrodinger" else 1
    eng = pinn_native.Engine([2, 20, 20, 20, 20, n_out], LB, UB, pde=pde, dtype=dtype)
    pts = lambda n: np.column_stack([rs.uniform(LB[0], UB[0], n), rs.uniform(LB[1], UB[1], n)])
    if pde != "burgers_ide":
        eng.set_collocation(pts(N_F))
    eng.set_data(pts(N_U), rs.standard_normal((N_U, n_out)))
    if pde in ("schrodinger", "adr", "adr_ide"):
        t = rs.uniform(LB[1], UB[1], (N_B, 1))
        eng.set_boundary(np.hstack([0 * t + LB[0], t]), np.hstack([0 * t + UB[0], t]))
    if pde in ("adr", "adr_ide"):
        eng.set_pde_params(*ADR_COEF)
    elif pde != "schrodinger":
        eng.set_pde_params(0.01 / np.pi)
    eng.set_weights(0.3 * rs.standard_normal(eng.n_params))
    return eng


def _with_extra(extra):
    """a float64 context on kernel path 7 that holds one extra"""
    rs = np.random.RandomState(11)
    eng = _context("burgers" if extra == "sa" else "adr")
    assert eng.kernel_path() == 7
    if extra == "sa":
        eng.sa_set_weights(np.ones(N_U), np.ones(N_F))
    elif extra == "pw":
        eng.pw_set()
    elif extra == "robin":
        eng.set_robin(np.column_stack([np.full(N_W, LB[0]), rs.uniform(LB[1], UB[1], N_W)]), 1.0, 0.5, 0.0)
    elif extra == "source":
        eng.set_source(rs.standard_normal(N_F))
    elif extra == "fields":
        eng.set_coef_fields(np.tile(ADR_COEF, (N_F, 1)) * rs.uniform(0.9, 1.1, (N_F, 6)))
    return eng


def _call_setter(eng, name):
    """the C entry point itself (the Python wrapper would refuse a count that differs from its own before it gets there)"""
    from pinn_native import _dp
    rs = np.random.RandomState(13)
    if name == "pinn_set_robin":
        X = np.ascontiguousarray(np.column_stack([np.full(N_W, LB[0]), rs.uniform(LB[1], UB[1], N_W)]))
        a, b, g = np.ones(N_W), np.full(N_W, 0.5), np.zeros(N_W)
        eng._check(eng._lib.pinn_set_robin(eng._h, _dp(X), _dp(a), _dp(b), _dp(g), N_W, N_W))
    elif name == "pinn_set_source":
        s = rs.standard_normal(N_F)
        eng._check(eng._lib.pinn_set_source(eng._h, _dp(s), N_F))
    else:
        K = np.ascontiguousarray(np.tile(ADR_COEF, (N_F, 1)))
        eng._check(eng._lib.pinn_set_coef_fields(eng._h, _dp(K), N_F))


def _bits(eng):
    loss, grad, terms = eng.loss_grad()
    return np.float64(loss).tobytes() + np.asarray(grad).tobytes() + np.asarray(terms).tobytes()


def _refused(eng, call, sentence, before):
    """the call fails with exactly this sentence as PINN_EUNSUPPORTED (-5), and loss, gradient and terms keep their bits"""
    import pinn_native
    with pytest.raises(pinn_native.PinnNativeError) as ei:
        call()
    assert str(ei.value) == "libpinn_hip: %s (code -5)" % sentence
    assert _bits(eng) == before


def test_every_refusal_among_the_extras_word_for_word():
    # 1. an extra is present: no communicator, and where it applies no other kernel path and no point weights
    for extra in ("sa", "pw", "robin", "source", "fields"):
        eng = _with_extra(extra)
        before = _bits(eng)
        _refused(eng, lambda: eng.comm_init(b"\0" * 128, 1, 0), "pinn_comm_init: " + SINGLE_DEVICE[extra], before)
        _refused(eng, lambda: eng.comm_xgmi_export(1, 0), "pinn_comm_xgmi_export: " + SINGLE_DEVICE[extra], before)
        if extra in PATH_7_ONLY:
            _refused(eng, lambda: eng.set_kernel_path(0), PATH_7_ONLY[extra], before)
            assert eng.kernel_path() == 7
        else:
            _refused(eng, lambda: eng.pw_set(), PW_SET[extra], before)
        if extra == "pw":      # 2. point weights are on: none of the three
            for name in SETTERS:
                _refused(eng, lambda: _call_setter(eng, name), BY_POINT_WEIGHTS[name], before)
        eng.close()
    # 3. the other kinds: adr_ide is named, the Burgers kinds and Schrodinger are not
    for pde in ("adr_ide", "burgers", "burgers_ide", "schrodinger"):
        eng = _context(pde)
        before = _bits(eng)
        for name in SETTERS:
            sentence = (ON_ADR_IDE if pde == "adr_ide" else ON_OTHER_KINDS)[name]
            _refused(eng, lambda: _call_setter(eng, name), sentence, before)
        eng.close()
    # 4. a context with a (one-rank) communicator
    eng = _context("adr")
    eng.comm_xgmi_export(1, 0)
    before = _bits(eng)
    for name in SETTERS:
        _refused(eng, lambda: _call_setter(eng, name), BY_COMMUNICATOR[name], before)
    _refused(eng, lambda: eng.pw_set(), "pinn_pw_set: point weights are single-device; this context has a communicator",
             before)
    eng.close()
    # 5. the two weight kinds away from their own kind of problem, path and dtype
    eng = _context("adr")
    _refused(eng, lambda: eng.sa_set_weights(np.ones(N_U), np.ones(N_F)),
             "pinn_sa_set_weights: self-adaptive weights are for Burgers inference (pde 0) only", _bits(eng))
    eng.set_kernel_path(0)
    _refused(eng, lambda: eng.pw_set(), "pinn_pw_set: point weights need kernel path 7 (this context runs path 0)",
             _bits(eng))
    eng.close()
    eng = _context("burgers")
    _refused(eng, lambda: eng.pw_set(), "pinn_pw_set: point weights are for the adr kind (pde 5) only", _bits(eng))
    eng.set_kernel_path(0)
    _refused(eng, lambda: eng.sa_adam_init(1e-3),
             "pinn_sa_adam_init: self-adaptive weights need kernel path 7 (this context runs path 0)", _bits(eng))
    eng.close()
    eng = _context("burgers", "f32")
    _refused(eng, lambda: eng.sa_set_weights(np.ones(N_U), np.ones(N_F)),
             "pinn_sa_set_weights: self-adaptive weights need float64", _bits(eng))
    eng.close()
    eng = _context("adr", "f32")
    _refused(eng, lambda: eng.pw_adam_init(1e-3), "pinn_pw_adam_init: point weights need float64", _bits(eng))
    eng.close()
