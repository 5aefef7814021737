"""CPU check of the tracks-pose boundary: the five entries are declared in include/orbx.h
with the reference lines they replace, exported by liborbx.so and listed in the binding's EXPORTS, and the binding
offers its method group."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("orbx_tracks_pose_device", "orbx_tracks_pose_results_device", "orbx_tracks_pose_fetch",
           "orbx_tracks_pose_pair_fetch", "orbx_tracks_pose")
CITES = ("src/feature_tracking.cpp:166-193", "src/feature_tracking.cpp:222-242", "src/feature_tracking.cpp:244-310",
         "src/with_bundle_adjustment.cpp:180-203")


def header():
    return open(os.path.join(ROOT, "include", "orbx.h")).read()


def test_the_five_entries_are_declared_exported_and_bound(pkg):
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = pkg.orbx.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
        assert name in pkg.orbx.EXPORTS, name


def test_the_declarations_cite_the_reference():
    src = header()
    section = src[src.index("rank 11"):]
    for cite in CITES:
        assert cite in section, cite
    # the comment in front of each declaration names at least one reference line
    for name in SYMBOLS:
        at = section.index("int %s(" % name)
        comment = section[:at].rsplit("/*", 1)[1]
        assert re.search(r"src/\w+\.cpp:\d+", comment) or name == "orbx_tracks_pose_results_device", name
    at = section.index("} orbx_tracks_pose_view;")
    assert re.search(r"src/\w+\.cpp:\d+", section[:at].rsplit("/* Device-side view", 1)[1])


def test_the_binding_offers_the_method_group(pkg):
    for m in ("tracks_pose", "tracks_pose_view", "tracks_pose_fetch", "tracks_pose_pair_fetch", "tracks_pose_window"):
        assert callable(getattr(pkg.Context, m)), m
    v = pkg.orbx.TracksPoseView
    assert C.sizeof(v) == 7 * 8 + 4 * 4 and v.slot_capacity.offset == 56 and v.n_pairs.offset == 68
