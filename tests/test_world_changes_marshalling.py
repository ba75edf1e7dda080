"""binding.WorldChanges' method bodies, without a device (the pattern of tests/test_binding_marshalling.py): every public
method marshals its smallest valid host-mode arguments into its C entry point on a map that was never created (h = None, a
null sdm_map *).  The entry point refuses the null map before it touches it, so the method must raise SdmError naming that
function with SDM_ERR_INVALID_ARGUMENT: not TypeError or ctypes.ArgumentError, and it must not return."""
import ctypes

import numpy as np
import pytest

from semantic_dsp_map_amd import binding as B

P1 = np.array([[0.5, 0.25, 0.125]], np.float32)
C1 = np.array([[1, 2, 3]], np.int32)

CASES = [
    ("update", "sdm_world_changes_update", lambda w: w.update()),
    ("update-every-option", "sdm_world_changes_update",
     lambda w: w.update(face_connected=True, by_label=True, static_only=True, observed_only=True, max_last_stamp=7, labels=(1, 255),
                        classes=(B.WORLD_CHANGE_VANISHED,), min_cells=3, max_cells=9)),
    ("regions", "sdm_get_world_changes", lambda w: w.regions()),
    ("cells", "sdm_get_world_change_cells", lambda w: w.cells()),
    ("cells-window", "sdm_get_world_change_cells", lambda w: w.cells(first=2, cap=3)),
    ("labels", "sdm_get_world_change_labels", lambda w: w.labels()),
    ("query", "sdm_query_world_changes", lambda w: w.query(xyz=P1)),
    ("query-cells", "sdm_query_world_changes", lambda w: w.query(cells=C1)),
]


@pytest.fixture(scope="module")
def unmade():
    """the client of an SdmMap that sdm_create never saw: the loaded library and a null handle"""
    g = object.__new__(B.SdmMap)
    g.L, g.h = B.load_library(), None
    return B.WorldChanges(g)


@pytest.mark.parametrize("method, c_name, call", CASES, ids=[c[0] for c in CASES])
def test_method_reaches_its_entry_point(unmade, method, c_name, call):
    with pytest.raises(B.SdmError) as e:
        call(unmade)
    assert not isinstance(e.value, (TypeError, ctypes.ArgumentError))
    assert str(e.value).startswith("%s failed: SDM_ERR_INVALID_ARGUMENT (" % c_name), str(e.value)


def test_cases_name_every_public_method():
    public = {n for n in vars(B.WorldChanges) if not n.startswith("_") and callable(getattr(B.WorldChanges, n))}
    assert {c[0].split("-")[0] for c in CASES} == public, sorted(public)
