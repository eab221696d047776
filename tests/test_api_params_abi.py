"""The binding's parameter builders, which need the built library for the defaults (as the other *_abi tests do): every
family takes its keywords over the library's defaults and refuses an unknown keyword, struct_size and reserved with its
own TypeError text."""
import ctypes as C

import pytest

from geometric_mapping_amd import api

# (builder, family word of the error text, a keyword it takes, whether its struct has a `reserved` field)
FAMILIES = (
    (api.GeometricMapping.surface_params, "surface", dict(n_sectors=12, up=(0, 1, 0)), True),
    (api.WallMap.params, "wall map", dict(n_sectors=12, point=(1, 2, 3)), True),
    (api.WallMap.region_params, "region", dict(min_cells=3), True),
    (api.WallMap.cloud_params, "cloud", dict(block_sectors=2, anchor=(1, 2, 3)), True),
    (api.WallMap.clearance_params, "clearance", dict(margin=0.25), True),
    (api.WallMap.section_params, "section", dict(harmonics=3), False),
    (api.WallMap.quantity_params, "quantity", dict(min_count=3), True),
    (api.WallMap.check_params, "check", dict(threshold=0.25), True),
    (api.WallMap.add_checked_params, "checked-add", dict(skip=1, min_delta=0.25), False),
    (api.WallMap.locate_params, "locate", dict(gate=0.25), True),
    (api.WallMap.align_params, "align", dict(clip=0.25), True),
    (api.WallMap.object_params, "object", dict(min_points=3), True),
)
MODULE_LEVEL = (("_wall_check_params", "check"), ("_wall_locate_params", "locate"), ("_wall_align_params", "align"),
                ("_wall_object_params", "object"), ("_wall_clearance_params", "clearance"), ("_wall_quantity_params", "quantity"),
                ("_wall_section_params", "section"), ("_wall_cloud_params", "cloud"))


@pytest.mark.parametrize("build,family,kw,has_reserved", FAMILIES, ids=[f[1] for f in FAMILIES])
def test_parameter_families_refuse_what_is_not_a_parameter(build, family, kw, has_reserved):
    p = build()
    assert p.struct_size == C.sizeof(type(p))          # the library's defaults, not an empty struct
    assert ("reserved" in dict(type(p)._fields_)) == has_reserved
    q = build(**kw)
    for k, v in kw.items():
        have = getattr(q, k)
        assert (list(have) == [float(x) for x in v]) if isinstance(have, C.Array) else (have == v), k
    for k in set(dict(type(p)._fields_)) - set(kw) - {"struct_size", "reserved"}:
        a, b = getattr(p, k), getattr(q, k)
        assert (list(a) == list(b)) if isinstance(a, C.Array) else (a == b or (a != a and b != b)), k
    for bad in ("no_such_parameter", "struct_size", "reserved"):
        with pytest.raises(TypeError) as e:
            build(**{bad: 1})
        assert str(e.value) == f"unknown {family} parameter {bad!r}"


@pytest.mark.parametrize("name,family", MODULE_LEVEL)
def test_module_level_builders_are_the_same_rule(name, family):
    with pytest.raises(TypeError) as e:
        getattr(api, name)(struct_size=1)
    assert str(e.value) == f"unknown {family} parameter 'struct_size'"
    assert getattr(api, name)().struct_size > 0
