"""cave_amd/_build.py: dependency files written by the preprocessor and the one staleness rule, on toy sources built
with g++ in a temporary root; then what the rule recorded for the library's own units.  mtimes are set, never waited for."""

from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from cave_amd import _build, _lib

T0 = 1_600_000_000  # the sources' mtime; a build's output is set to T0 + 100, "newer" is T0 + 200


def _write(path, text, t=T0):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text)
    os.utime(path, (t, t))


def _touch(path, t=T0 + 200):
    os.utime(path, (t, t))


class Toy:
    """root/src dir/{main.c -> a.h -> b.h, other.h, new.h} -> root/out/main.o; `sub`: the directory of the sources"""

    def __init__(self, root, sub="src"):
        self.root, self.sub = str(root), sub
        self.src = self.path("main.c")
        self.out = os.path.join(self.root, "out", "main.o")
        _write(self.src, '#include <stdio.h>\n#include "a.h"\nint main(void) { return A + B; }\n')
        _write(self.path("a.h"), '#include "b.h"\n#define A 1\n')
        _write(self.path("b.h"), "#define B 2\n")
        _write(self.path("other.h"), "#define OTHER 3\n")
        _write(self.path("new.h"), "#define NEW 4\n")
        os.makedirs(os.path.dirname(self.out))

    def path(self, name):
        return os.path.join(self.root, self.sub, name)

    def rel(self, *names):
        return {os.path.join(self.sub, n) for n in names}

    def build(self, t=T0 + 100):
        """bring out up to date; -> whether the compiler ran (the output then gets mtime `t`)"""
        ran = _build.stale(self.out, self.root)
        _build.make(["g++", "-std=c++17", "-DTOY=1", "-c", self.src, "-o", self.out], self.src, self.out, root=self.root)
        if ran:
            _touch(self.out, t)
        return ran

    def deps(self):
        return set(_build.read_deps(self.out))


@pytest.fixture
def toy(tmp_path):
    t = Toy(tmp_path / "root")
    assert t.build()
    return t


def test_build_records_what_the_preprocessor_read(toy):
    assert not _build.stale(toy.out, toy.root)
    assert not toy.build()  # (and nothing runs again)
    assert toy.deps() == toy.rel("main.c", "a.h", "b.h")  # b.h: included by a.h only; stdio.h: outside the root
    assert not any(os.path.isabs(d) or d.startswith(os.pardir) for d in toy.deps())
    text = open(toy.out + ".d").read()
    assert text.startswith(os.path.join("out", "main.o") + ":") and toy.root not in text


def test_newer_transitive_header_is_stale_unrelated_file_is_not(toy):
    _touch(toy.path("other.h"))
    assert not _build.stale(toy.out, toy.root)
    _touch(toy.path("b.h"), T0 + 100)  # as old as the output: up to date (>=)
    assert not _build.stale(toy.out, toy.root)
    _touch(toy.path("b.h"))
    assert _build.stale(toy.out, toy.root)
    assert toy.build(T0 + 300)
    assert not _build.stale(toy.out, toy.root)


def test_new_include_is_picked_up(toy):
    """what a hand-kept list gets wrong: the source gains a header nobody wrote down"""
    _write(toy.src, '#include "a.h"\n#include "new.h"\nint main(void) { return A + B + NEW; }\n', T0 + 200)
    assert _build.stale(toy.out, toy.root)
    assert toy.build(T0 + 300)
    assert toy.deps() == toy.rel("main.c", "a.h", "b.h", "new.h")
    assert not _build.stale(toy.out, toy.root)
    _touch(toy.path("new.h"), T0 + 400)
    assert _build.stale(toy.out, toy.root)


def test_missing_or_truncated_dependency_file_is_stale(toy):
    saved = open(toy.out + ".d").read()
    os.remove(toy.out + ".d")
    assert _build.stale(toy.out, toy.root)
    open(toy.out + ".d", "w").close()
    assert _build.stale(toy.out, toy.root)
    with open(toy.out + ".d", "w") as fh:
        fh.write(saved)
    assert not _build.stale(toy.out, toy.root)
    os.remove(toy.out)
    assert _build.stale(toy.out, toy.root)


def test_deleted_header_is_stale_and_the_compiler_reports_it(toy, capfd):
    os.remove(toy.path("b.h"))
    assert _build.stale(toy.out, toy.root)
    with pytest.raises(subprocess.CalledProcessError) as e:  # (what a failed compile raises in every builder)
        toy.build()
    assert e.value.cmd[0] == "g++"
    err = capfd.readouterr().err
    assert "b.h" in err and "No such file" in err and "Traceback" not in err
    assert _build.stale(toy.out, toy.root)


def test_copied_tree_is_up_to_date(toy, tmp_path):
    there = str(tmp_path / "elsewhere" / "copy")
    shutil.copytree(toy.root, there)  # (copy2: mtimes preserved)
    out = os.path.join(there, "out", "main.o")
    assert not _build.stale(out, there)
    _touch(os.path.join(there, "src", "a.h"))
    assert _build.stale(out, there) and not _build.stale(toy.out, toy.root)


def test_path_with_a_space_round_trips(tmp_path):
    t = Toy(tmp_path / "a root", sub="my src#1")
    assert t.build()
    assert t.deps() == t.rel("main.c", "a.h", "b.h")  # the compiler's escapes, parsed; ours, written and parsed
    assert "my\\ src\\#1" in open(t.out + ".d").read()
    assert not _build.stale(t.out, t.root)
    _touch(t.path("b.h"))
    assert _build.stale(t.out, t.root)
    names = ["x y/a b.h", "c$d.h", "e#f.h", "plain.h"]
    _build.write_deps(t.out, [os.path.join(t.root, n) for n in names] + ["/usr/include/stdio.h"], t.root)
    assert _build.read_deps(t.out) == names
    assert _build.parse("o.o: a\\ b.c \\\n  c.h\\\n d.h\n# e.h: f.h\no.o: c.h g$$.h\n") == ["a b.c", "c.h", "d.h", "g$.h"]


# ---- the library's own units: three facts of the preprocessor's fan-out (not the whole table: it grows with every unit)
@pytest.fixture(scope="module")
def unit_deps():
    _lib.build()
    return {u: set(_build.read_deps(os.path.join(_lib._OBJ_DIR, u + ".o"))) for u in _lib._UNITS}


def _users(unit_deps, header):
    return {u for u, deps in unit_deps.items() if header in deps}


def test_cone_entry_h_is_read_by_the_host_unit_only(unit_deps):
    assert _users(unit_deps, "cave_amd/csrc/cone_entry.h") == {"cave_hip"}


def test_apgd_h_is_read_by_its_three_units(unit_deps):
    assert _users(unit_deps, "cave_amd/csrc/apgd.h") == {"cave_hip", "k_apgd_w1", "k_apgd_w4"}


def test_every_unit_reads_the_common_header_and_the_c_abi(unit_deps):
    for header in ("cave_amd/csrc/cone_common.h", "include/cave_hip.h"):
        assert _users(unit_deps, header) == set(_lib._UNITS), header
    for u, deps in unit_deps.items():
        assert f"cave_amd/csrc/{u}.hip" in deps and not _build.stale(os.path.join(_lib._OBJ_DIR, u + ".o")), u
