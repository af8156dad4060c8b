"""The host-side plan headers (plain C++ under csrc/ and include/) are tested through small stand-alone driver programs:
this module compiles one with the host compiler and runs it.  Plain module: no GPU, no tt_sketch_amd."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tt_sketch_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


def compile_driver(tmp_path_factory, name, source, extra=()):
    """-> the executable (a pathlib.Path in a fresh temporary directory `name`, where the caller may keep its case files).
    source: the program text, or the path of an existing .cpp; extra: flags after the base list."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    if "clang" in os.path.basename(cxx):                   # links its sanitizer runtimes statically as it is
        extra = [x for x in extra if not x.startswith("-static-lib")]
    d = tmp_path_factory.mktemp(name)
    exe = d / "driver"
    if str(source).endswith(".cpp"):
        src = source
    else:
        src = d / "driver.cpp"
        src.write_text(source)
    done = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", CSRC, "-I", INCLUDE, "-o", str(exe), str(src)],
                          capture_output=True, text=True)
    assert done.returncode == 0, "%s does not compile:\n%s" % (name, done.stderr[-4000:])
    return exe


def run_driver(exe, args=(), stdin=None, env=None, with_stderr=False):
    """-> the program's standard output (with_stderr: the pair (stdout, stderr)); a nonzero exit status fails with the end
    of its standard error"""
    done = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True, env=env)
    assert done.returncode == 0, "%s: exit status %d\n%s\n%s" % (exe, done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return (done.stdout, done.stderr) if with_stderr else done.stdout
