"""_analysis.bind_out: an output struct of the library bound to the arrays it is to fill.

Every result class's ``out()`` is a call of it.  Held here, without the library: each pointer field holds its own
array's address, under the field's declared pointer type; a wrong dtype and a non-contiguous array are refused;
an optional output that is not there leaves a null field.
"""
import ctypes as C

import numpy as np
import pytest

from mbb_emcee_amd import (_analysis, _native, diagnostics, draws, evidence, goodness, loo, marginals, optimize, predict,
                           results)

# (the result class's arrays, its struct, field name -> attribute name where the two differ)
CASES = {
    "summary": (lambda: results._Raw(3, 2), _native.SummaryOut, {}),
    "diagnostics": (lambda: diagnostics._Raw(3, 4), _native.DiagOut, {}),
    "marginals": (lambda: marginals._Raw(3, 6, 4, 2), _native.MarginalsOut, {}),
    "predict": (lambda: predict._Raw(3, 4, 2), _native.PredictOut, {}),
    "goodness": (lambda: goodness._Raw(3, 4, 2), _native.GoodnessOut, {}),
    "loo": (lambda: loo._Raw(3, 4), _native.PointwiseOut, {}),
    "evidence": (lambda: evidence._Raw(3, 5, 7, True), _native.EvidenceOut, {"n2_inside": "n_inside"}),
    "optimize": (lambda: optimize._Raw(3, 4, 5), _native.MapOut, {}),
    "draws": (lambda: draws._Raw(3, 4, ("peaklambda", "dustmass")), _native.DrawsOut, {}),
}


def _address(pointer):
    return C.cast(pointer, C.c_void_p).value


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_pointer_field_holds_its_arrays_address(name):
    make, struct, renamed = CASES[name]
    raw = make()
    o = raw.out()
    assert type(o) is struct
    seen = 0
    for field, ctype in struct._fields_:
        if issubclass(ctype, C.Array):                       # draws: a pointer per derived column, null where absent
            assert field == "derived"
            for k, d in enumerate(draws._DERIVED_ORDER):
                a = raw.derived.get(d)
                assert _address(o.derived[k]) == (None if a is None else a.ctypes.data)
                seen += a is not None
            continue
        a = getattr(raw, renamed.get(field, field))
        assert isinstance(a, np.ndarray) and a.size > 0, field
        assert type(getattr(o, field)) is ctype
        assert _address(getattr(o, field)) == a.ctypes.data, field
        assert a.dtype == np.dtype(ctype._type_), field
        seen += 1
    assert seen >= 5


def test_wrong_dtype_is_a_type_error():
    raw = results._Raw(2, 3)
    raw.mean = np.zeros(raw.mean.shape, dtype=np.float32)
    with pytest.raises(TypeError, match="SummaryOut.mean"):
        raw.out()
    with pytest.raises(TypeError):
        _analysis.bind_out(_native.PredictOut, {"n_used": np.zeros(4, dtype=np.int32)})       # int32 for an int64 *
    with pytest.raises(TypeError):
        _analysis.bind_out(_native.MarginalsOut, {"counts1": np.zeros(4, dtype=np.int32)})    # int32 for a uint32 *
    with pytest.raises(TypeError):
        _analysis.bind_out(_native.DiagOut, {"tau": [0.0, 1.0]})                              # not an array at all
    with pytest.raises(TypeError):
        _analysis.bind_out(_native.DrawsOut, {"derived": [None, np.zeros(3, dtype=np.float32), None]})


def test_non_contiguous_array_is_a_value_error():
    raw = goodness._Raw(3, 4, 2)
    raw.ml_model = np.zeros((4, 3)).T                        # the right shape and dtype, strided
    assert raw.ml_model.shape == (3, 4) and not raw.ml_model.flags.c_contiguous
    with pytest.raises(ValueError, match="GoodnessOut.ml_model"):
        raw.out()
    with pytest.raises(ValueError):
        _analysis.bind_out(_native.DiagOut, {"tau": np.zeros(10)[::2]})
    for n in (2, 4):                                         # a field of three pointers takes three entries
        with pytest.raises(ValueError, match="DrawsOut.derived"):
            _analysis.bind_out(_native.DrawsOut, {"derived": [np.zeros(3)] * n})


def test_none_and_missing_leave_a_null_pointer():
    o = diagnostics._Raw(2, 0).out()                         # no autocorrelation curve asked for
    assert not o.acf and o.tau and o.status
    o = evidence._Raw(2, 5, 7, False).out()                  # the draws are not kept
    assert not o.prop and not o.prop_lnprob and not o.prop_lnq and not o.post_lnq
    assert o.lnz and o.n1 and o.n2_inside and o.prop_cov
    o = _analysis.bind_out(_native.PredictOut, {"mean": np.zeros(3), "min": None, "no_such_field": 5})
    assert o.mean and not o.min and not o.n_used and not o.status
    o = draws._Raw(2, 3).out()
    assert not any(bool(o.derived[k]) for k in range(3)) and o.rows
