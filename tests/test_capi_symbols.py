"""CPU: the C-ABI library loads and exports every symbol include/*.h declares."""
import ctypes
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        text = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names |= set(re.findall(r"\b(cloudaae_[a-z0-9_]+)\s*\(", text))
    return sorted(names)


def test_library_exports_every_declared_symbol():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    path = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(path)
    declared = _declared()
    assert len(declared) >= 8
    assert "cloudaae_fc_plan" in declared       # the path query tests/test_35_fc_paths_gpu.py states its coverage with
    # the variant queries tests/test_49_point_op_variants_gpu.py names its cases with
    for query in ("cloudaae_farthest_point_sample_variant", "cloudaae_knn_variant", "cloudaae_nn_distance_variant"):
        assert query in declared
    missing = [n for n in declared if not hasattr(lib, n)]
    assert not missing, missing
    # one ABI revision: the header's, the library's and what the Python host read from the header (cloudaae_amd/_lib.py)
    header = open(os.path.join(ROOT, "include", "cloudaae_hip.h")).read()
    abi = int(re.search(r"#define\s+CLOUDAAE_ABI_VERSION\s+(\d+)", header).group(1))
    assert lib.cloudaae_version() == abi
    from cloudaae_amd import _lib
    assert _lib.ABI_VERSION == abi


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cloudaae_hip.h")).read(), flags=re.S)


def test_header_declares_every_exported_definition():
    """The converse: a CLOUDAAE_API definition without a prototype is checked by no compiler (a definition that disagrees
    with its extern "C" prototype does not compile) and typed by nobody (the Python host types calls from the header)."""
    defined = set()
    for src in glob.glob(os.path.join(ROOT, "cloudaae_amd", "csrc", "*.hip")):
        defined |= set(re.findall(r"\bCLOUDAAE_API\b[\w\s*]*?\b(cloudaae_[a-z0-9_]+)\s*\(", open(src).read()))
    assert len(defined) >= 185
    undeclared = sorted(defined - set(_declared()))
    assert not undeclared, undeclared


def test_reader_covers_the_header():
    """cloudaae_amd/_lib.py types every call from the header's text: its reader finds exactly the names the plain search
    above finds, every one of them is typed on the loaded library, and a name the header lacks is refused, not handed
    out untyped."""
    import pytest
    from cloudaae_amd import _lib
    assert sorted(_lib._PROTOTYPES) == _declared()       # (the typedef cloudaae_allreduce_fn is no `name(`: in neither)
    L = _lib.lib()
    for name, (restype, argtypes) in _lib._PROTOTYPES.items():
        fn = getattr(L._cdll, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes and fn.restype is restype, name
        assert getattr(L, name) is fn or getattr(L, name).fn is fn, name
    with pytest.raises(AttributeError, match="cloudaae_no_such_entry is not declared"):
        L.cloudaae_no_such_entry


def test_signatures_are_the_prototypes_that_take_a_stream():
    from cloudaae_amd import _lib
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    streamed = {name for name, args in re.findall(r"\b(cloudaae_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header())
                if "cloudaae_stream_t" in args}
    assert len(streamed) >= 132 and set(_lib._SIGNATURES) == streamed
    for name, sig in _lib._SIGNATURES.items():
        assert sig is _lib._PROTOTYPES[name][1] and _lib._PROTOTYPES[name][0] is I, name
    # rows whose shapes exercise the reader: a trailing plain pointer, const char *, a pointer result, (void) with a
    # long long result, pointers to const pointers, and the by-value unsigned types
    assert _lib._PROTOTYPES["cloudaae_fc_plan"] == (I, [I] * 7 + [P])
    assert _lib._PROTOTYPES["cloudaae_set_knob"] == (I, [ctypes.c_char_p, I])
    assert _lib._PROTOTYPES["cloudaae_last_error"] == (ctypes.c_char_p, [])
    assert _lib._PROTOTYPES["cloudaae_side_stream"] == (P, [])
    assert _lib._PROTOTYPES["cloudaae_mean_workspace_bytes"] == (LL, [])
    assert _lib._PROTOTYPES["cloudaae_crc32c"] == (ctypes.c_uint, [P, ctypes.c_ulonglong, ctypes.c_uint])
    assert _lib._SIGNATURES["cloudaae_edgeconv_revlists"] == [I, I, I, I, P, P, P]
    assert _lib._SIGNATURES["cloudaae_zero_buffers"] == [I, P, P, P]
    for query in ("cloudaae_fc_plan", "cloudaae_set_knob", "cloudaae_side_stream", "cloudaae_mean_workspace_bytes"):
        assert query not in _lib._SIGNATURES


def test_struct_layouts_are_the_c_compiler_s(tmp_path):
    """tests/abi_layout_main.c, compiled against the header, prints sizeof and every offsetof of the three structs the
    Python host fills; the ctypes classes built from the header's text must lay their fields out the same way."""
    import shutil
    import subprocess
    import pytest
    from cloudaae_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on this machine")
    exe = str(tmp_path / "abi_layout")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi_layout_main.c"), "-o", exe], check=True)
    printed = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        struct, field, value = line.split()
        printed.setdefault(struct, []).append((field, int(value)))
    classes = {"cloudaae_gemm_tn_job": _lib.GemmTnJob, "cloudaae_bn_sync": _lib.BnSyncStruct,
               "cloudaae_fc_layer": _lib.FcLayer}
    assert sorted(printed) == sorted(classes)
    for struct, cls in classes.items():
        want = [("sizeof", ctypes.sizeof(cls))] + [(name, getattr(cls, name).offset) for name, _ in cls._fields_]
        assert printed[struct] == want, struct       # same fields, same order, same offsets
    assert [len(c._fields_) for c in classes.values()] == [11, 4, 30]
    assert _lib.BnSyncStruct._fields_[0] == ("allreduce", _lib.ALLREDUCE_FN)


_TINY_HEADER = """
#define CLOUDAAE_ABI_VERSION 7
typedef void *cloudaae_stream_t; /* hipStream_t */
typedef int (*cloudaae_allreduce_fn)(void *ctx, double *buf, int count, cloudaae_stream_t stream);
typedef struct cloudaae_pair {
    int a, b;
    const float *x, *y;   /* two declarators */
    cloudaae_allreduce_fn fn;
} cloudaae_pair;
const char *cloudaae_name(void);
int cloudaae_run(int n, const cloudaae_pair *pairs, const int *const *lists,
                 cloudaae_stream_t stream);
%s
"""


def test_reader_refuses_what_it_does_not_know():
    import pytest
    from cloudaae_amd import _lib
    I, P = ctypes.c_int, ctypes.c_void_p
    abi, structs, prototypes, launching = _lib.read_header(_TINY_HEADER % "")
    assert abi == 7 and structs == {"cloudaae_pair": [("a", I), ("b", I), ("x", P), ("y", P), ("fn", _lib.ALLREDUCE_FN)]}
    assert prototypes == {"cloudaae_name": (ctypes.c_char_p, []), "cloudaae_run": (I, [I, P, P, P])}
    assert launching == {"cloudaae_run"}
    for extra, offender in (
            # a type without a ctypes counterpart: of a parameter, of the result, of a field; a struct by value
            ("int cloudaae_bad_type(int n, size_t bytes);", r"cloudaae_bad_type\(size_t bytes\)"),
            ("short cloudaae_bad_result(int n);", "result of cloudaae_bad_result"),
            ("int cloudaae_unnamed(int, float *x);", r"cloudaae_unnamed\(int\)"),
            ("typedef struct cloudaae_bad_field {\n    int n;\n    size_t bytes;\n} cloudaae_bad_field;",
             "struct cloudaae_bad_field, field bytes"),
            ("int cloudaae_by_value(cloudaae_pair pair);", r"cloudaae_by_value\(cloudaae_pair pair\)"),
            ("int cloudaae_text(char *out);", r"cloudaae_text\(char \*out\)"),
            # a declaration in a form the prototype pattern misses: a function-pointer parameter, a definition, one cut
            # by the preprocessor, a nested struct
            ("int cloudaae_callback(int n, int (*fn)(int), cloudaae_stream_t stream);", "mentions cloudaae_callback"),
            ("int cloudaae_inline(int n) { return n; }", "mentions cloudaae_inline"),
            ("int cloudaae_split(int n,\n#ifdef WIDE\n long long m\n#else\n int m\n#endif\n);",
             r"cloudaae_split\(long long m int m\)"),
            ("typedef struct cloudaae_nest {\n    struct { int a; } in;\n} cloudaae_nest;", "struct cloudaae_nest")):
        with pytest.raises(_lib.HipLibraryError, match=offender):
            _lib.read_header(_TINY_HEADER % extra)
    # the callback type is the one thing the reader takes from Python: a header that changes it is refused
    with pytest.raises(_lib.HipLibraryError, match="cloudaae_allreduce_fn no longer"):
        _lib.read_header((_TINY_HEADER % "").replace("double *buf, int count", "double *buf, long long count"))
    with pytest.raises(_lib.HipLibraryError, match="CLOUDAAE_ABI_VERSION"):
        _lib.read_header("int cloudaae_version(void);")


def test_header_is_plain_c():
    # no torch / C++ types may leak into the boundary
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        text = open(h).read()
        assert "torch" not in text.lower().replace("pytorch", "")
        assert "std::" not in text and "at::" not in text


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "cloudaae_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(root, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f
                assert "liboracle" not in text, f


def test_fc_ticket_is_taken_after_the_atomics_are_drained():
    """csrc/fc.hip, a product cut over K (and over row tiles) and finished by the last workgroup to arrive: every
    wave must wait for what it publishes -- the agent-scope stores of its partial tile -- with s_waitcnt vmcnt(0)
    BEFORE the barrier that precedes the ticket: s_barrier does not drain the counter, and a ticket published
    early lets the last workgroup read incomplete sums.
    Checked on the emitted gfx950 ISA: between the last publishing instruction (global_store_dword ... sc1) and
    the ticket (global_atomic_add ... sc0) there is an s_waitcnt vmcnt(0) in front of the s_barrier; and the
    partial tiles are read back with agent-scope loads (sc1)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        import pytest
        pytest.skip("no hipcc on this machine")
    src = os.path.join(ROOT, "cloudaae_amd", "csrc", "fc.hip")
    asm = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                          "-munsafe-fp-atomics", "-S", "--cuda-device-only", src, "-o", "-"],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    tickets = [i for i, l in enumerate(asm) if re.search(r"\bglobal_atomic_add\s.*\bsc0\b", l)]
    assert len(tickets) >= 6, "expected a ticket per instantiation of the forward body in fc.hip's ISA"
    publish = re.compile(r"global_store_dword\s.*\bsc1\b")
    kinds = set()
    for t in tickets:
        pubs = [i for i in range(t) if publish.search(asm[i])]
        assert pubs, "ticket without preceding publication"
        kinds.add("store")
        window = [l.strip() for l in asm[pubs[-1] + 1:t]]
        bar = [i for i, l in enumerate(window) if l.startswith("s_barrier")]
        assert bar, "no barrier between the publication and the ticket"
        waits = [i for i, l in enumerate(window[:bar[0]]) if re.match(r"s_waitcnt\s+vmcnt\(0\)", l)]
        assert waits, "the publication is not drained before the barrier:\n" + "\n".join(window)
    assert kinds == {"store"}, kinds
    assert any(re.search(r"buffer_load_dwordx4\s.*\bsc1\b", l) for l in asm), "partial tiles not read at agent scope"
