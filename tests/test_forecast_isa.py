"""The kernels of the forecast (forecast.hip) use no scratch and spill no register, vector or scalar.  Reads the code
object's metadata only.  (tests/test_isa_hygiene.py scans the object for FLAT memory instructions, like every other unit of
the library.)"""
from tests.test_isa_hygiene import device_elf, hip_units, kernels_meta
from tests.test_reach_isa import sgpr_spills

# "k_query_forecastE": the point query's name ends there in its mangled form (the E closes the anonymous namespace), which
# keeps k_query_forecast_segments from matching it too
FORECAST_KERNELS = ("k_forecast_classify", "k_forecast_scatter", "k_forecast_reduce", "k_forecast_cells_count", "k_forecast_cells_write",
                    "k_query_forecastE", "k_query_forecast_segments")


def test_the_unit_is_listed():
    assert "forecast" in hip_units()


def test_forecast_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    elf = device_elf(tmp_path, "forecast")
    meta, spills = kernels_meta(elf), sgpr_spills(elf)
    assert len([n for n in meta if "k_forecast_" in n or "k_query_forecast" in n]) == len(FORECAST_KERNELS), list(meta)
    for k in FORECAST_KERNELS:
        found = [(n, v) for n, v in meta.items() if k in n]
        assert len(found) == 1, (k, list(meta))
        name, v = found[0]
        assert int(v["private_segment_fixed_size"]) == 0 and int(v["vgpr_spill_count"]) == 0, (k, v)
        assert spills[name] == 0, (k, spills[name])
