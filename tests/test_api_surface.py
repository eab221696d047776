"""The binding's surface without the library: every public module-level name of geometric_mapping_amd.api, every public
method of its five classes and the underscore names that tests, tools and the benchmark reach still exist with the
signature tests/golden/api_surface.json recorded.  New names are allowed; a recorded one may not leave or change."""
import inspect
import json
import os

from geometric_mapping_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_surface.json")
CLASSES = ("GeometricMapping", "GeometricMappingGroup", "WallMap", "WallAlignmentRule", "WallAlignment")
# underscore names somebody outside api.py reaches (tests/, tools/, bench.py, examples/, __init__.py)
PRIVATE_MODULE = ("_f32", "_dptr", "_wall_elements", "_ADD_CHECKED_INFO")
PRIVATE_METHODS = ("_pose", "_add_info", "_check_info", "_locate_info", "_add_checked_info", "_u8", "_surface", "_fetch",
                   "_check", "_h", "_borrowed")


def _describe(obj):
    """The signature of a callable, else the kind of thing the name holds."""
    if isinstance(obj, property):
        return "<property>"
    if callable(obj):
        try:
            return str(inspect.signature(obj))
        except (TypeError, ValueError):
            return "<callable>"
    return f"<{type(obj).__name__}>"


def surface():
    out = {}
    for name, obj in vars(api).items():
        if inspect.ismodule(obj) or name == "annotations":
            continue
        if not name.startswith("_") or name in PRIVATE_MODULE:
            out[name] = _describe(obj)
    for cname in CLASSES:
        cls = getattr(api, cname)
        for name in dir(cls):
            if name.startswith("__") or (name.startswith("_") and name not in PRIVATE_METHODS):
                continue
            static = inspect.getattr_static(cls, name)
            out[f"{cname}.{name}"] = _describe(static if isinstance(static, property) else getattr(cls, name))
    return out


def record_golden():
    """Not collected: writes the golden file from the api.py that is importable (run on the commit to hold to)."""
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")


def test_every_recorded_name_keeps_its_signature():
    with open(GOLDEN) as f:
        want = json.load(f)
    have = surface()
    assert len(want) > 200
    missing = sorted(set(want) - set(have))
    assert not missing, missing
    changed = {k: (want[k], have[k]) for k in want if have[k] != want[k]}
    assert not changed, changed


def test_the_names_others_reach_are_recorded():
    with open(GOLDEN) as f:
        want = json.load(f)
    for k in PRIVATE_MODULE + ("WallMap._pose", "WallMap._add_info", "WallMap._check_info", "WallMap._locate_info",
                               "WallMap._add_checked_info", "WallMap._borrowed", "WallMap._h", "GeometricMapping._u8",
                               "GeometricMapping._surface", "GeometricMapping._fetch", "GeometricMapping._check",
                               "GeometricMappingGroup._fetch", "GeometricMappingGroup._check", "WallAlignment._h"):
        assert k in want, k


if __name__ == "__main__":
    record_golden()
