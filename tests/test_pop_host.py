"""The host side of kh_pop_bubbles_into without a device: the symbol is declared, exported, bound with five arguments, in the Rust crate
and in INTEGRATION.md; the KH_POP_* words of the header agree with the Python and Rust constants and, in the first eight, with the
KH_CLIP_* words; the kernels and the comparator exist; the ABI version is still 2; and the command line is untouched -- the feature's
interface is the library, `kmerust --help` prints the recorded bytes."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
NAME = "kh_pop_bubbles_into"
WORDS = ("UNITIGS", "CANDIDATES", "POPPED", "POPPED_KMERS", "POPPED_COUNT", "KEPT_KMERS", "KEPT_COUNT", "LINKS", "BUBBLES")
CLIP_WORDS = ("UNITIGS", "CANDIDATES", "CLIPPED", "CLIPPED_KMERS", "CLIPPED_COUNT", "KEPT_KMERS", "KEPT_COUNT", "LINKS")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbol_declared_mapped_and_bound():
    from krust_amd import native
    header = re.sub(r"/\*.*?\*/", "", _read("include", "kmerhip.h"), flags=re.S)
    mapfile = _read("krust_amd", "csrc", "kmerhip.map")
    rust = _read("bindings", "rust", "src", "lib.rs")
    assert re.search(r"\bint\s+%s\s*\(kh_ctx \*dst, kh_ctx \*src, uint64_t min_count, uint64_t max_kmers, uint64_t \*out\s*\)" % NAME, header), \
        f"{NAME} is not declared in kmerhip.h"
    assert NAME in mapfile and re.search(r"global:\s*kh_\*;", mapfile)
    assert NAME in native.SYMBOLS and len(native.SYMBOLS[NAME][1]) == 5 and native.SYMBOLS[NAME] == native.SYMBOLS["kh_clip_tips_into"]
    assert re.search(r"pub fn %s\(" % NAME, rust) and re.search(r"pub fn pop_bubbles_into\(", rust)
    assert re.search(r"\bfn %s\(" % NAME, _read("INTEGRATION.md"))
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header) and native.ABI_VERSION == 2
    assert callable(native.DeviceCounter.pop_bubbles_into)
    assert re.search(r"KH_HD bool kh_pop_beats\(", _read("krust_amd", "csrc", "unitig_bits.h"))
    unitig = _read("krust_amd", "csrc", "unitig.hip")
    for kernel in ("pop_exits_kernel", "pop_decide_kernel", "clip_keep_kernel"):
        assert re.search(r"\bvoid %s\(" % kernel, unitig), kernel
    assert re.search(r'extern "C" int %s\(' % NAME, unitig)
    assert re.search(r"static_assert\(KH_POP_KEPT_KMERS == KH_CLIP_KEPT_KMERS && KH_POP_KEPT_COUNT == KH_CLIP_KEPT_COUNT", unitig)


def test_the_library_exports_the_symbol():
    import ctypes as C
    from krust_amd import native
    native.lib()
    for so in ("libkmerhip.so", "libkmerhip_testing.so"):
        assert hasattr(C.CDLL(os.path.join(os.path.dirname(native.LIB_PATH), so)), NAME), so


def test_header_words_agree_with_the_bindings_and_with_clip():
    from krust_amd import native
    header = _read("include", "kmerhip.h")
    rust = _read("bindings", "rust", "src", "lib.rs")
    assert int(re.search(r"#define\s+KH_POP_WORDS\s+(\d+)", header).group(1)) == native.POP_WORDS == len(WORDS) == len(native.POP_NAMES) == 9
    assert re.search(r"pub const POP_WORDS: usize = 9;", rust)
    for i, w in enumerate(WORDS):
        assert int(re.search(r"#define\s+KH_POP_%s\s+(\d+)" % w, header).group(1)) == i == getattr(native, "POP_" + w)
        assert native.POP_NAMES[i] == w.lower()
        assert re.search(r"pub const POP_%s: usize = %d;" % (w, i), rust)
    for i, w in enumerate(CLIP_WORDS):                                   # words 0 to 7 mean what the KH_CLIP_* words of the same index mean
        assert int(re.search(r"#define\s+KH_CLIP_%s\s+(\d+)" % w, header).group(1)) == i
        assert WORDS[i] == w.replace("CLIPPED", "POPPED")


def test_the_default_bound_is_two_k():
    import inspect
    from krust_amd import native
    sig = inspect.signature(native.DeviceCounter.pop_bubbles_into)
    assert [p.default for p in list(sig.parameters.values())[2:]] == [1, None]
    assert re.search(r"mk = 2 \* self\.k if max_kmers is None", inspect.getsource(native.DeviceCounter.pop_bubbles_into))


def test_the_command_line_is_untouched():
    """No `kmerust pop`, no `clip --bubbles`: --help is the recorded one, byte for byte, and the host layer does not name the entry."""
    with open(os.path.join(ROOT, "tests", "golden", "cli_surface.json")) as f:
        golden = json.load(f)["vectors"][json.dumps(["--help"])]
    p = subprocess.run([BIN, "--help"], stdin=subprocess.DEVNULL, capture_output=True, cwd=ROOT, timeout=60)
    assert {"status": p.returncode, "stdout": p.stdout.decode("latin-1"), "stderr": p.stderr.decode("latin-1")} == golden
    assert golden["status"] == 0 and "pop" not in golden["stdout"].replace("population", "")
    for f in ("kmerust.cpp", "kmerust_host.cpp", "kmerust_host.h", "cli_args.h"):
        assert NAME not in _read("krust_amd", "host", f), f
    assert NAME not in _read("tests", "host_asan", "stub_kmerhip.cpp")
