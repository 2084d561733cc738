"""When a native piece of this project is rebuilt: dependency files written by the compiler's own preprocessor, and the
one staleness rule every builder asks.

An output `out` keeps `out + ".d"` beside it: a Make rule naming the files the preprocessor read for it, as paths
relative to the repository root (files outside the root are dropped), so a built tree may be copied elsewhere with its
mtimes.  The file comes from a preprocessor run of its own, with the -D / -I / -std / offload flags of the compile
command, and is written before the compile starts; the compile command itself runs as the builder gives it.
"""

from __future__ import annotations

import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEP_FLAGS = ("-D", "-I", "-std=", "--offload-arch=")  # what of a compile command decides which files are read
_WORD = re.compile(r"(?:\\[ #]|\S)+")  # a word of a Make rule: an escaped space does not end it
_ESCAPE = re.compile(r"\\([ #])|\$\$")


def parse(text: str) -> list:
    """the prerequisites of the Make rules in `text`, each once, in order (line continuations, `\\ `, `\\#`, `$$`)"""
    deps = []
    for line in text.replace("\\\r\n", " ").replace("\\\n", " ").splitlines():
        if line.lstrip().startswith("#"):  # (hipcc brackets the rule of each offload target in comment lines)
            continue
        words = [_ESCAPE.sub(lambda m: m.group(1) or "$", w) for w in _WORD.findall(line)]
        ends = [k for k, w in enumerate(words) if w.endswith(":")]  # (an unescaped space splits a target, not the rule)
        deps += words[ends[0] + 1:] if ends else []
    return list(dict.fromkeys(deps))


def _quote(path: str) -> str:
    return path.replace("$", "$$").replace("#", "\\#").replace(" ", "\\ ")


def write_deps(out: str, files, root: str = ROOT) -> None:
    """out + ".d": one rule, `out` and the `files` under `root` relative to it; replaces the file in one step"""
    root = os.path.abspath(root)
    rel = [os.path.relpath(os.path.abspath(f), root) for f in [out, *files]]
    inside = [r for r in rel[1:] if not r.startswith(os.pardir + os.sep)]
    with open(out + ".d.tmp", "w") as fh:
        fh.write(_quote(rel[0]) + ":" + "".join(" \\\n  " + _quote(r) for r in dict.fromkeys(inside)) + "\n")
    os.replace(out + ".d.tmp", out + ".d")


def read_deps(out: str) -> list:
    """the files `out + ".d"` names, relative to the root; OSError if there is no such file"""
    with open(out + ".d") as fh:
        return parse(fh.read())


def stale(out: str, root: str = ROOT) -> bool:
    """Is `out` to be rebuilt: it or its dependency file is missing or unreadable, or a file named there is missing or
    newer than `out`."""
    try:
        built = os.stat(out).st_mtime
        deps = read_deps(out)
        return not deps or any(os.stat(os.path.join(root, d)).st_mtime > built for d in deps)
    except (OSError, UnicodeError):
        return True


def older(out: str, inputs) -> bool:
    """the link rule: `out` is missing or older than one of `inputs`"""
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in inputs)


def run(cmd, src: str, out: str, verbose: bool = False, root: str = ROOT) -> None:
    """Build `out` from `src` by `cmd`, which runs as it is; before it, the preprocessor of the same compiler writes the
    dependency file (an interrupted build then leaves `out` older than the edit, or no dependency file)."""
    dep_cmd = [cmd[0], *[a for a in cmd[1:] if a.startswith(_DEP_FLAGS)], "-MM", "-MT", out,
               "-Wno-unused-command-line-argument", src]
    r = subprocess.run(dep_cmd, check=True, stdout=subprocess.PIPE, text=True)  # (the compiler's errors go to stderr)
    write_deps(out, [os.path.abspath(f) for f in parse(r.stdout)], root)
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def make(cmd, src: str, out: str, force: bool = False, verbose: bool = False, root: str = ROOT) -> str:
    """`out`, rebuilt by run() where it is stale (or `force`)"""
    if force or stale(out, root):
        run(cmd, src, out, verbose, root)
    return out
