"""Builds tests/host_driver/host_text_driver.cpp with the host sources that need no device library, once per test
session and per variant, and runs it as a child process.

  "san"    g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -fopenmp
  "plain"  the product's own flags (epa_ng_amd/build.py HOST_FLAGS: -O2), so that optimised code is compared too

One `g++ -c` per source, at most 16 at a time.  Measured with seven sources compiling side by side: 6 s for the
sanitized build, 2.5 s for the plain one (io.cpp is the longest single compile of both).  Objects and the program are
kept under tests/_build/host_driver/<variant>-<hash of sources and flags>/ (git-ignored), so a second session with
unchanged sources builds nothing again.

The driver is an ordinary child process: nothing is preloaded, no Python process loads sanitized code, and the driver
opens no GPU.  ASAN_OPTIONS=detect_leaks=1 stays on.  Where g++ cannot link a sanitized hello-world the sanitized
variant is skipped with the linker's message."""
import hashlib
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "epa_ng_amd", "csrc", "host")
DRIVER = os.path.join(ROOT, "tests", "host_driver", "host_text_driver.cpp")
# the host sources that need no device library
SOURCES = ["io.cpp", "tree.cpp", "model.cpp", "aa_models.cpp", "parse_model.cpp", "fastq.cpp"]
SAN_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-std=c++17", "-fopenmp"]
# the sanitizers' runtime is linked INTO the driver: a dynamically linked one refuses to start unless it is the first
# library the loader brings in, which depends on the environment the suite runs in
SAN_LINK = ["-static-libasan", "-static-libubsan"]
VARIANTS = ("san", "plain")
MAX_JOBS = 16
RUN_TIMEOUT = 20.0   # seconds per driver run: a hang is a failure

_built = {}


def _flags(variant):
    if variant == "san":
        return SAN_FLAGS
    from epa_ng_amd import build
    return list(build.HOST_FLAGS)


def _sanitizer_links():
    """None when `g++ -fsanitize=address,undefined` links and runs a hello-world, else the reason"""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "hello.cpp"), os.path.join(d, "hello")
        with open(src, "w") as f:
            f.write("#include <cstdio>\nint main() { std::puts(\"hello\"); return 0; }\n")
        r = subprocess.run(["g++"] + SAN_FLAGS + SAN_LINK + [src, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            return "g++ -fsanitize=address,undefined cannot link a hello-world: " + r.stderr.strip()[-400:]
        r = subprocess.run([exe], capture_output=True, text=True)
        if r.returncode != 0 or r.stdout.strip() != "hello":
            return "a sanitized hello-world does not run: " + r.stderr.strip()[-400:]
    return None


def _build_dir(variant, key):
    for base in (os.path.join(ROOT, "tests", "_build", "host_driver"), None):
        try:
            if base is None:
                return tempfile.mkdtemp(prefix="host_driver_" + variant + "_")
            d = os.path.join(base, variant + "-" + key)
            os.makedirs(d, exist_ok=True)
            probe = os.path.join(d, ".w")
            open(probe, "w").close()
            os.remove(probe)
            return d
        except OSError:
            continue


def driver(variant, host_dir=HOST):
    """path of the driver built as `variant`; host_dir: another copy of the host sources (an earlier revision dropped
    into the same driver)"""
    memo = (variant, host_dir)
    if memo in _built:
        if isinstance(_built[memo], Exception):
            raise _built[memo]
        return _built[memo]
    if variant == "san":
        why = _sanitizer_links()
        if why:
            pytest.skip(why)
    flags = _flags(variant)
    srcs = [DRIVER] + [os.path.join(host_dir, s) for s in SOURCES]
    h = hashlib.sha256(" ".join(flags + SAN_LINK).encode())
    for p in srcs + [os.path.join(host_dir, "epa_host.hpp"), os.path.join(ROOT, "include", "epa_dev.h")]:
        with open(p, "rb") as f:
            h.update(f.read())
    bdir = _build_dir(variant, h.hexdigest()[:16])
    exe = os.path.join(bdir, "host_text_driver")
    if not os.path.exists(exe):
        inc = ["-I", os.path.join(ROOT, "include"), "-I", host_dir]

        def compile_one(src):
            obj = os.path.join(bdir, os.path.basename(src)[:-4] + ".o")
            r = subprocess.run(["g++"] + flags + inc + ["-c", src, "-o", obj], capture_output=True, text=True)
            return obj, r
        try:
            with ThreadPoolExecutor(max_workers=min(MAX_JOBS, len(srcs))) as pool:
                done = list(pool.map(compile_one, srcs))
            for obj, r in done:
                if r.returncode != 0:
                    raise RuntimeError("g++ failed on %s:\n%s" % (obj, r.stderr[-4000:]))
            r = subprocess.run(["g++"] + flags + (SAN_LINK if variant == "san" else []) + [o for o, _ in done] + ["-o", exe + ".tmp"],
                               capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("linking the host driver failed:\n" + r.stderr[-4000:])
            os.replace(exe + ".tmp", exe)
        except RuntimeError as e:
            _built[memo] = e
            raise
    _built[memo] = exe
    return exe


def run(variant, args, timeout=RUN_TIMEOUT, host_dir=HOST, check=True):
    """runs the driver; returns its stdout lines.  Asserts exit status 0 and an empty stderr (a sanitizer report goes to
    stderr and makes the status non-zero); a run longer than `timeout` seconds raises subprocess.TimeoutExpired"""
    exe = driver(variant, host_dir)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    env.setdefault("OMP_NUM_THREADS", "8")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=timeout, env=env)
    if check:
        assert r.returncode == 0 and r.stderr == b"", (variant, args[:3], r.returncode, r.stderr.decode(errors="replace")[-3000:])
        return r.stdout.decode(errors="replace").split("\n")[:-1]
    return r


def unhex(s):
    return b"" if s == "-" else bytes.fromhex(s)
