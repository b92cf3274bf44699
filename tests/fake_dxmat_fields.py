"""``tests/fake_dxmat.py`` with the per-point parameter-field entry points of the C ABI (``dxm_set_param_field``,
``dxm_param_field_mask``, ``dxm_algorithmic_bytes``): the handle keeps the fields, validates them with the rules of
``csrc/dxmat.hip::dxm_set_param_field`` and integrates with the array-parameter restatement of the oracle
(``tests/param_fields_ref.py``).  TEST INFRASTRUCTURE ONLY, like the class it wraps."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import FakeDxmat, _addr
from param_fields_ref import j2_update_fields


class FakeDxmatFields(FakeDxmat):
    def __init__(self, real):
        super().__init__(real)
        self.field_calls = []     # (handle, param_index, values | None) of every accepted dxm_set_param_field

    def dxm_set_param_field(self, h, idx, host):
        m = self._h(h)
        if m.law not in (_lib.LAW_J2_LINEAR, _lib.LAW_J2_VOCE):
            return self._fail(-1, "per-point parameter fields exist for DXM_LAW_J2_LINEAR and DXM_LAW_J2_VOCE only")
        if not 0 <= idx < len(m.params):
            return self._fail(-1, f"law {m.law} has no parameter {idx}")
        fields = m.__dict__.setdefault("fields", {})
        a = _addr(host)
        if not a:
            if idx in fields:
                del fields[idx]
                m.epoch += 1
            self.field_calls.append((_addr(h), idx, None))
            return 0
        v = np.array(np.ctypeslib.as_array((C.c_double * max(m.n, 1)).from_address(a))[: m.n])
        for i, x in enumerate(v):
            if not np.isfinite(x):
                return self._fail(-1, f"parameter {idx} is not finite at point {i}")
            if idx == 0 and not x > 0.0:
                return self._fail(-1, f"invalid elastic constant E={x:g} at point {i}")
            if idx == 1 and not -1.0 < x < 0.5:
                return self._fail(-1, f"invalid elastic constant nu={x:g} at point {i}")
        fields[idx] = v
        m.epoch += 1
        self.field_calls.append((_addr(h), idx, v))
        return 0

    def dxm_param_field_mask(self, h):
        return sum(1 << i for i in self._h(h).__dict__.get("fields", {}))

    def dxm_algorithmic_bytes(self, h):
        f = self._h(h).__dict__.get("fields", {})
        streams = (2 if (0 in f or 1 in f) else 0) + sum(1 for i in f if i >= 2)
        return 496 + 8 * streams

    def _update(self, m, grad):
        f = m.__dict__.get("fields", {})
        if not f:
            return super()._update(m, grad)
        m.io_valid[1] = 0
        s0 = m.state[0]
        prm = [f.get(i, m.params[i]) for i in range(len(m.params))]
        kind = "linear" if m.law == _lib.LAW_J2_LINEAR else "voce"
        r = j2_update_fields(grad, s0["epsp"], s0["p"], kind, *prm)
        m.state[1] = dict(p=r["p"].copy(), epsp=r["epsp"].copy())
        m.s1_alias = False
        m.launched = True
        m.stats = dict(n_points=m.n, n_plastic=int(r["plastic"].sum()), n_not_converged=0, n_nan=0, max_local_iters=0)
        r["n_plastic"], r["n_not_converged"] = m.stats["n_plastic"], 0
        return r
