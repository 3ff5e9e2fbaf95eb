"""What the six pattern objects share on the host (hisparse_amd/csrc/pattern_object.h), through ctypes on the HIP library: the codes of
destroy / info / set_stream / sync on NULL, and the create-time error text, which every family keeps for itself per thread.  No kernel
is launched: every create here is refused by its argument checks.  The same scaffolding over a fake runtime, failures included:
tests/cpp/test_staging.cpp (test_tiles_cpu.py::test_staging)."""
import ctypes as C

import numpy as np
import pytest

from hisparse_amd import attention, attention_backward, heads, pattern, rows, wide

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_MATRIX = -1, -4

# a 6 x 9 pattern of 7 entries, and the same with an indptr that decreases
INDICES = np.array([0, 4, 8, 2, 3, 5, 7], dtype=np.uint32)
INDPTR = np.array([0, 3, 3, 4, 5, 6, 7], dtype=np.uint32)
DOWN = np.array([0, 3, 2, 4, 5, 6, 7], dtype=np.uint32)

# family -> (the module that binds it, the arguments of its create between device_id and the arrays, those after the arrays)
FAMILIES = {
    "hsp": (pattern, (0, 6, 9), (4,)),
    "hsr": (rows, (6,), None),      # hsr_create takes indptr alone
    "hsw": (wide, (6, 9), (1,)),
    "hsat": (attention, (6, 9), ()),
    "hsab": (attention_backward, (6, 9), ()),
    "hsmh": (heads, (6, 9), (2, 1)),
}


def _call(family, name):
    return getattr(FAMILIES[family][0].lib(), f"{family}_{name}")


def _create(family, out, indptr):
    _, before, after = FAMILIES[family]
    arrays = (indptr.ctypes.data,) if after is None else (indptr.ctypes.data, INDICES.ctypes.data)
    return _call(family, "create")(out, 0, *before, *arrays, *(after or ()))


def _text(family):
    return _call(family, "last_error")(None).decode()


@pytest.mark.parametrize("family", FAMILIES)
def test_null_object(family):
    assert _call(family, "destroy")(None) == 0
    assert _call(family, "info")(None, None, None) == BAD_ARG
    nnz, device_bytes = C.c_uint64(11), C.c_uint64(12)
    assert _call(family, "info")(None, C.byref(nnz), C.byref(device_bytes)) == BAD_ARG and (nnz.value, device_bytes.value) == (11, 12)
    assert _call(family, "set_stream")(None, None) == BAD_ARG
    assert _call(family, "sync")(None) == BAD_ARG


@pytest.mark.parametrize("family", FAMILIES)
def test_refused_create_sets_the_familys_text(family):
    assert _create(family, None, INDPTR) == BAD_ARG
    assert _text(family) == ("null rows pointer" if family == "hsr" else "null pattern pointer")
    h = C.c_void_p(0xBAD)
    assert _create(family, C.byref(h), DOWN) == BAD_MATRIX and not h.value
    assert _text(family) and "null" not in _text(family)


@pytest.mark.parametrize("first", FAMILIES)
def test_another_familys_refusal_leaves_the_text_alone(first):
    h = C.c_void_p(0xBAD)
    assert _create(first, C.byref(h), DOWN) == BAD_MATRIX and not h.value
    kept = _text(first)
    assert kept and "null" not in kept
    for other in FAMILIES:
        if other != first:
            assert _create(other, None, INDPTR) == BAD_ARG
            assert _text(other).startswith("null ") and _text(first) == kept, (first, other)
    # and a refusal of its own replaces it
    assert _create(first, None, INDPTR) == BAD_ARG and _text(first) != kept
