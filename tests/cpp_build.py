"""The one g++ command line of the C++ facade's test programs (tests/cpp/*.cpp, shared header tests/cpp/facade_test.h): build_program(name) gives
tests/cpp/bin/<name>, rebuilt only when the source, a header or a linked library is newer.  One set of flags for every program; liboracle.so and the
stream-gate library are linked on request."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP_DIR = os.path.join(ROOT, "tests", "cpp")
BIN_DIR = os.path.join(CPP_DIR, "bin")
LIB_DIR = os.path.join(ROOT, "deeppowers_amd")
ORACLE_DIR = os.path.join(ROOT, "oracle")
ROCM_LIB = "/opt/rocm/lib"
HEADERS = [os.path.join(CPP_DIR, "facade_test.h"), os.path.join(ROOT, "include", "deeppowers", "fhe.hpp"), os.path.join(ROOT, "include", "dpfhe.h")]


def libraries(oracle=False, gate=False):
    """(directory, -l flag) of what a program links, the project's own first; builds the two optional ones"""
    libs = [(LIB_DIR, "-ldpfhe_api"), (LIB_DIR, "-ldpfhe_hip")]
    if oracle:
        subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, "liboracle.so"])
        libs.append((ORACLE_DIR, "-loracle"))
    if gate:
        import stream_gate
        libs.append((os.path.dirname(stream_gate.build_library()), "-lstream_gate"))
    return libs + [(ROCM_LIB, "-lamdhip64")]


def command(src, exe, libs=None, extra_flags=()):
    """the g++ line that compiles `src` against the facade and links it into `exe`"""
    libs = libraries() if libs is None else libs
    dirs = list(dict.fromkeys(d for d, _ in libs))
    return (["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", *extra_flags, str(src), "-o", str(exe)]
            + [f for d, l in libs for f in ("-L" + d, l)] + [f"-Wl,-rpath,{d}" for d in dirs])


def build_program(name, *, oracle=False, gate=False, extra_flags=()):
    """tests/cpp/<name>.cpp -> tests/cpp/bin/<name>"""
    src, exe = os.path.join(CPP_DIR, name + ".cpp"), os.path.join(BIN_DIR, name)
    libs = libraries(oracle, gate)
    deps = [src] + HEADERS + [os.path.join(d, f"lib{l[2:]}.so") for d, l in libs if d != ROCM_LIB]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(BIN_DIR, exist_ok=True)
        subprocess.check_call(command(src, exe, libs, extra_flags))
    return exe
