"""The binder of the C ABI (mtad-gat-pytorch_amd/_abi.py) without a GPU: the header parser on small literal headers, the
declarations it makes on the built library against lists written out by hand, the Structures and constants of the package
against include/mtadgat.h, and the convention tests/pointer_proxy.py relies on."""
import ctypes

import pytest

import _abi
import _native
import streaming

vp, ci, i32, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
f32, f64, u64, u32 = ctypes.c_float, ctypes.c_double, ctypes.c_uint64, ctypes.c_uint32
P = ctypes.POINTER


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


@pytest.fixture(scope="module")
def header():
    return _native._HEADER


def _one(text, **kw):
    (entry,) = _abi.Header(text).register(**kw).prototypes.items()
    name, (restype, params, _) = entry
    return name, restype, params


# ---- the parser on literal headers -------------------------------------------------------------------------------------------
def test_a_prototype_broken_over_three_lines():
    name, restype, params = _one("int mtadgat_thing(mtadgat_handle h, const float* x_dev,\n"
                                 "                  int64_t batch,\n"
                                 "                  size_t workspace_bytes, void* stream);\n")
    assert name == "mtadgat_thing" and restype is ci
    assert params == [("h", vp), ("x_dev", vp), ("batch", i64), ("workspace_bytes", sz), ("stream", vp)]


def test_comments_are_stripped_inside_the_parameter_list_too():
    name, restype, params = _one("/* int mtadgat_not_this(int a); */\n"
                                 "int mtadgat_q(const double* q_host, int nq, float* out_dev /* (nq, count, d) */, void* stream); // end\n")
    assert name == "mtadgat_q" and params == [("q_host", P(f64)), ("nq", ci), ("out_dev", vp), ("stream", vp)]


def test_void_parameter_list_and_scalar_results():
    assert _one("int mtadgat_chunk(void);") == ("mtadgat_chunk", ci, [])
    assert _one("uint32_t mtadgat_key(float value, int descending);") == ("mtadgat_key", u32, [("value", f32), ("descending", ci)])
    assert _one("size_t mtadgat_x_bytes(int64_t n, int32_t d, uint64_t seed, double a);")[1:] == (
        sz, [("n", i64), ("d", i32), ("seed", u64), ("a", f64)])
    assert _one("const char* mtadgat_name(int slot);")[1] is ctypes.c_char_p
    assert _one("int64_t mtadgat_start(int64_t count);")[1] is i64


def test_pointer_classes():
    _, _, params = _one("int mtadgat_p(double ms[MTADGAT_SLOTS], int64_t launches[4], const void* const* tensors_dev,\n"
                        "              const unsigned char* label_dev, uint8_t* flags_dev, const char* name, mtadgat_handle* out,\n"
                        "              int64_t* count_host, const int64_t* n_elements, const int32_t* dims_host);")
    assert params == [("ms", P(f64)), ("launches", P(i64)), ("tensors_dev", vp), ("label_dev", vp), ("flags_dev", vp),
                      ("name", ctypes.c_char_p), ("out", P(vp)), ("count_host", P(i64)), ("n_elements", vp), ("dims_host", P(i32))]


def test_defines_structs_and_registered_structures():
    text = ("#ifndef MTADGAT_H\n#define MTADGAT_H\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
            "#define MTADGAT_N 3\n"
            "typedef enum mtadgat_status { MTADGAT_OK = 0, MTADGAT_ERR = -1 /* bad */ } mtadgat_status;\n"
            "typedef struct mtadgat_rec { float lo, hi; /* two */ int32_t n; const float* w[MTADGAT_N]; uint8_t* f; } mtadgat_rec;\n"
            "typedef struct mtadgat_handle_s* mtadgat_handle;\n"
            "int mtadgat_a(const mtadgat_rec* rec, const mtadgat_rec* rec_dev);\n"
            "#ifdef __cplusplus\n}\n#endif\n#endif\n")

    class Rec(ctypes.Structure):
        _fields_ = [("lo", f32), ("hi", f32), ("n", i32), ("w", vp * 3), ("f", vp)]

    h = _abi.Header(text).register(mtadgat_rec=Rec)
    assert h.defines == {"MTADGAT_N": 3}
    assert h.structs == {"mtadgat_rec": list(Rec._fields_)}
    assert h.prototypes["mtadgat_a"][:2] == (ci, [("rec", P(Rec)), ("rec_dev", P(Rec))])
    # unregistered, the struct is known by name only: a device record passes as an address, anything else is refused
    with pytest.raises(ValueError, match=r"mtadgat_rec\*.*`rec`.*int mtadgat_a\("):
        _abi.Header(text).register()
    assert _abi.Header(text.replace("const mtadgat_rec* rec, ", "")).register().prototypes["mtadgat_a"][1] == [("rec_dev", vp)]

    class Drifted(ctypes.Structure):
        _fields_ = [("lo", f32), ("hi", f32), ("n", i64), ("w", vp * 3), ("f", vp)]
    with pytest.raises(ValueError, match="Drifted does not mirror mtadgat_rec"):
        _abi.Header(text).register(mtadgat_rec=Drifted)


@pytest.mark.parametrize("text, quoted", [
    ("int mtadgat_u(int n, long double x);", "long double"),
    ("int mtadgat_u(int n, short* v_dev);", "short"),
    ("int mtadgat_u(int n, float** rows_dev[4]);", "rows_dev"),
    ("int mtadgat_u(int n, const char** names);", "names"),
    ("void mtadgat_u(int n);", "void"),
    ("int mtadgat_u(int n, int (*callback)(int));", "callback"),
    ("int mtadgat_u(int, float);", "int"),
    ("int other_u(int n);", "other_u"),
])
def test_what_the_binder_does_not_know_raises_with_the_prototype(text, quoted):
    with pytest.raises(ValueError) as e:
        _abi.Header(text).register()
    assert quoted in str(e.value) and text.rstrip(";") in str(e.value)


# ---- the declarations on the built library -------------------------------------------------------------------------------------
EXPECTED = {
    "mtadgat_forward_series": ([vp, vp, i64, vp, i64, i64, i64, vp, vp, vp, vp, sz, vp], ci),
    "mtadgat_fit_prepare": ([vp, i64, vp, f64, f64, f64, f64, ci, vp, vp, i64, vp, sz, vp], ci),
    "mtadgat_eval_window_sse": ([vp, vp, i64, ci, ci, vp, i64, ci, i64, vp, i64, i64, vp, ci, vp, vp, vp, sz, vp], ci),
    "mtadgat_backward": ([vp, vp, i64, i64, f32, u64, vp, vp, vp, sz, vp, vp, sz, vp], ci),
    # ... and the typed host pointers
    "mtadgat_create": ([P(_native.Config), P(vp)], ci),
    "mtadgat_load_weights": ([vp, P(_native.Params), vp], ci),
    "mtadgat_eval_runs": ([vp, vp, i64, f64, ci, i64, i64, i64, vp, sz, vp, vp, P(i64), vp], ci),
    "mtadgat_stream_init": ([vp, vp, i64, i64, f64, f64, i64, i64, P(i32), P(f32), P(f32), vp], ci),
    "mtadgat_stream_flush": ([vp, vp, i64, i64, vp, i64, ci, P(streaming._Outputs), vp], ci),
    "mtadgat_read_packed": ([vp, P(f32), i64, vp], ci),
    "mtadgat_profile_read": ([vp, P(f64), P(i64)], ci),
    "mtadgat_selfcheck_gather_table": ([vp, P(_native.Params), vp], i64),
    "mtadgat_set_option": ([vp, ctypes.c_char_p, ci], ci),
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_end_to_end_mapping(lib, name):
    argtypes, restype = EXPECTED[name]
    fn = getattr(lib, name)
    assert list(fn.argtypes) == argtypes and fn.restype is restype


def test_return_types(lib, header):
    assert lib.mtadgat_eval_order_key.restype is u32
    assert lib.mtadgat_stream_window_start.restype is i64
    assert lib.mtadgat_last_error.restype is ctypes.c_char_p and lib.mtadgat_abi_version.restype is ci
    sizes = [n for n in header.prototypes if n.endswith(("_bytes", "_scratch"))]
    assert len(sizes) >= 25
    for n in sizes:
        assert getattr(lib, n).restype is sz, n


def test_every_declared_function_is_exported_and_bound(lib, header):
    assert len(header.prototypes) >= 129
    for name, (restype, params, text) in header.prototypes.items():
        assert hasattr(lib, name), f"{name} is declared in include/mtadgat.h but the library does not export it"
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params) == (text.count(",") + 1 if params else 0), text
        assert fn.restype is restype and restype is not None


def test_structures_mirror_the_header(header):
    for cls, name, size in ((_native.Config, "mtadgat_config", 56), (_native.Params, "mtadgat_params", 8 * (12 + 10 * 8)),
                            (streaming._Outputs, "mtadgat_stream_outputs", 64)):
        assert list(cls._fields_) == header.structs[name], name                # names, order and types
        assert ctypes.sizeof(cls) == sum(ctypes.sizeof(t) for _, t in header.structs[name]) == size, name
    per_layer = [t for _, t in _native.Params._fields_ if t is not vp]
    assert len(per_layer) == 10 and all(t is vp * header.defines["MTADGAT_MAX_LAYERS"] for t in per_layer)
    assert header.structures == {"mtadgat_config": _native.Config, "mtadgat_params": _native.Params,
                                 "mtadgat_stream_outputs": streaming._Outputs}


def test_constants_come_from_the_header(lib, header):
    assert header.defines == {"MTADGAT_ABI_VERSION": 1, "MTADGAT_MAX_LAYERS": 8, "MTADGAT_FIT_STATE_FIELDS": 8, "MTADGAT_PROFILE_SLOTS": 6}
    assert _native.ABI_VERSION == 1 and _native.MAX_LAYERS == 8 and _native.PROFILE_SLOTS == 6 and len(_native.FIT_STATE_FIELDS) == 8
    assert lib.mtadgat_abi_version() == _native.ABI_VERSION


def test_pointer_proxy_convention(header):
    """tests/pointer_proxy.py holds c_void_p arguments to the arena as device pointers and leaves typed pointers alone: in the
    evaluation, parts, SPOT and prep sections a pointer parameter is c_void_p exactly when its name does not end in _host."""
    seen = 0
    for name, (_, params, text) in header.prototypes.items():
        if not name.startswith(("mtadgat_eval_", "mtadgat_spot_", "mtadgat_prep_")):
            continue
        decls = [d.strip() for d in text[text.index("(") + 1:-1].split(",")] if params else []
        for (pname, t), decl in zip(params, decls):
            assert decl.endswith(pname), (name, decl)
            if "*" in decl:
                assert (t is vp) == (not pname.endswith("_host")), (name, decl)
                assert t is vp or t in (P(f64), P(i64)), (name, decl)
                seen += 1
            else:
                assert t in (ci, i64, sz, f32, f64), (name, decl)
    assert seen >= 150
