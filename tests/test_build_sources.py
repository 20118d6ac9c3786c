"""build.SOURCES / build.HEADERS list exactly the files of csrc/: a file left
out of them is neither compiled nor covered by source_hash()."""
import os

from agi_lidar_slam_amd import build


def test_every_csrc_file_is_listed():
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp", ".hpp"))}
    listed = set(build.SOURCES) | set(build.HEADERS)
    assert on_disk - listed == set()


def test_every_listed_file_exists():
    listed = build.SOURCES + build.HEADERS
    assert len(set(listed)) == len(listed)
    missing = [f for f in listed if not os.path.isfile(os.path.join(build.CSRC, f))]
    assert missing == []
    assert all(f.endswith((".hip", ".cpp")) for f in build.SOURCES)
    assert all(f.endswith(".hpp") for f in build.HEADERS)
