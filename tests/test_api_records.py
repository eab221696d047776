"""The binding's records without the library: every record dtype of api.py is its ctypes struct's (one statement of the
layout, in _lib.py) with the size include/gm_hip.h gives it, and the derived info tuples are their struct's fields.
The parameter builders, which need the built library for the defaults, are in tests/test_api_params_abi.py."""
import ctypes as C

import numpy as np
import pytest

from geometric_mapping_amd import _lib, api

RECORDS = (
    ("RAW_CELL", "WallRawCell", 24), ("REGION", "WallRegion", 64), ("WALL_ALIGN_SCORE", "WallAlignScore", 24),
    ("WALL_CHECK_POINT", "WallCheckPoint", 32), ("WALL_CLEARANCE_CELL", "WallClearanceCell", 16),
    ("WALL_CLEARANCE_RUN", "WallClearanceRun", 72), ("WALL_CLEARANCE_STATION", "WallClearanceStation", 32),
    ("WALL_CLOUD_POINT", "WallCloudPoint", 40), ("WALL_OBJECT", "WallObject", 128), ("WALL_QUANTITY", "WallQuantity", 88),
    ("WALL_QUANTITY_RUN", "WallQuantityRun", 136), ("WALL_SECTION", "WallSection", 144),
    ("WALL_SECTION_SUMS", "WallSectionSums", 448), ("_CELL", "SurfaceCell", 16),
)
INFOS = (("_CHECK_INFO", "WallCheckInfo"), ("_CLEARANCE_INFO", "WallClearanceInfo"), ("_CLOUD_INFO", "WallCloudInfo"),
         ("_OBJECTS_INFO", "WallObjectsInfo"), ("_QUANTITIES_INFO", "WallQuantitiesInfo"), ("_REGION_METRICS", "WallRegionMetrics"),
         ("_SECTIONS_INFO", "WallSectionsInfo"))


@pytest.mark.parametrize("name,struct,size", RECORDS)
def test_record_dtype_is_its_structs(name, struct, size):
    dt, st = getattr(api, name), getattr(_lib, struct)
    assert isinstance(dt, np.dtype) and dt == np.dtype(st)
    assert dt.itemsize == size == C.sizeof(st)
    assert list(dt.names) == [k for k, _t in st._fields_]
    assert [dt.fields[k][1] for k in dt.names] == [getattr(st, k).offset for k in dt.names]


def test_the_fourteen_records_are_all_of_them():
    assert len(RECORDS) == 14
    have = {k for k, v in vars(api).items() if isinstance(v, np.dtype) and v.names}
    assert have == {r[0] for r in RECORDS}
    assert api.WALL_MESH_TRIANGLE == np.dtype("<u4") and C.sizeof(_lib.WallMeshTriangle) == 12


@pytest.mark.parametrize("name,struct", INFOS)
def test_derived_info_tuples_are_the_structs_fields(name, struct):
    fields = [k for k, _t in getattr(_lib, struct)._fields_]
    assert list(getattr(api, name)) == [k for k in fields if k not in ("struct_size", "reserved")]
    assert _lib.info_fields(getattr(_lib, struct)) == getattr(api, name)


def test_hand_written_info_tuples_name_fields_of_their_structs():
    for names, struct in ((api._ADD_CHECKED_INFO, _lib.WallAddCheckedInfo), (api._ALIGN_INT + api._ALIGN_F64, _lib.WallAlignInfo),
                          (api._MESH_INFO, _lib.WallMeshInfo), (api._REGION_INFO, _lib.WallRegionsInfo),
                          (api._WALL_VEC, _lib.WallParams)):
        fields = [k for k, _t in struct._fields_]
        assert set(names) <= set(fields) and len(set(names)) == len(names)
    assert "reserved" in api._ADD_CHECKED_INFO
