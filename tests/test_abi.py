"""CPU-side checks of the drop-in boundary: the shared library builds for gfx950, loads, and
exports exactly the entry points include/selfrecon_hip.h declares (no compute without a GPU)."""
import ctypes
import os
import re
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = []
    for fn in os.listdir(os.path.join(ROOT, "include")):
        if fn.endswith(".h"):
            txt = open(os.path.join(ROOT, "include", fn)).read()
            names += re.findall(r"^\s*(?:int|const char\*|int64_t)\s+(sr_\w+)\s*\(", txt, flags=re.M)
    return sorted(set(names))


def _defines():
    """{name: value} of the integer `#define SR_*` lines of the header, in file order (a later one may use an earlier one)."""
    vals = {}
    txt = open(os.path.join(ROOT, "include", "selfrecon_hip.h")).read()
    for name, expr in re.findall(r"^[ \t]*#define[ \t]+(SR_\w+)[ \t]+([^/\n]+?)[ \t]*(?:/\*.*)?$", txt, flags=re.M):
        if re.fullmatch(r"[\w \t()+*-]+", expr) and not re.search(r"[a-z]", expr):
            vals[name] = int(eval(expr, {"__builtins__": {}}, dict(vals)))
    return vals


def test_library_builds_and_exports_every_declared_symbol():
    from selfreconcode_amd.build import build_lib
    lib = ctypes.CDLL(build_lib(verbose=False))
    decl = _declared()
    assert len(decl) >= 12
    missing = [n for n in decl if not hasattr(lib, n)]
    assert not missing, missing


def test_python_binding_covers_the_header():
    from selfreconcode_amd import _lib
    decl = set(_declared()) - {"sr_abi_version", "sr_build_arch", "sr_build_digest"}
    assert decl == set(_lib.SIGNATURES), decl ^ set(_lib.SIGNATURES)
    assert _lib.build_arch() == "gfx950" and _lib.abi_version() >= 1
    from selfreconcode_amd import build
    assert _lib.build_digest() == build._digest() == build.embedded_digest()      # the loaded library is the one these sources describe


def test_no_cpu_fallback():
    """The HIP operators must refuse CPU tensors instead of silently computing elsewhere."""
    import torch
    from selfreconcode_amd.ext import FastMinv, GridSamplerMine
    with pytest.raises(RuntimeError):
        FastMinv.Fast3x3Minv(torch.eye(3).view(1, 3, 3))
    with pytest.raises(RuntimeError):
        GridSamplerMine.forward(torch.zeros(1, 2, 3, 3, 3), torch.zeros(1, 1, 1, 4, 3), 0, 1)


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under selfreconcode_amd/ may reference it."""
    bad = []
    for dp, _, fns in os.walk(os.path.join(ROOT, "selfreconcode_amd")):
        for fn in fns:
            if fn.endswith(".py"):
                txt = open(os.path.join(dp, fn)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "/root/reference" in txt:
                    bad.append(os.path.join(dp, fn))
    assert not bad, bad


def _struct_bodies():
    """{typedef name: body} of the header's structs, in both spellings it uses, by this file's own reading (comments removed)."""
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "selfrecon_hip.h")).read(), flags=re.S)
    bodies = {name: body for body, name in re.findall(r"typedef\s+struct\s*\{([^{}]*)\}\s*(sr_\w+)\s*;", txt)}
    tagged = dict(re.findall(r"(?<!typedef )struct\s+(\w+)\s*\{([^{}]*)\}\s*;", txt))
    bodies.update({name: tagged[tag] for tag, name in re.findall(r"typedef\s+struct\s+(\w+)\s+(sr_\w+)\s*;", txt)})
    assert len(re.findall(r"\bstruct\b", txt)) == len(bodies) + len(tagged)          # every `struct` of the header is one of these
    return bodies


def _flat_fields(cls):
    return [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _ in cls._fields_]


def test_ctypes_structs_have_the_size_the_header_declares(tmp_path):
    """Every argument struct crosses the boundary by pointer or by value: the ctypes classes _lib builds from the header and the C
    declarations must agree (gcc compiles the header as plain C -- it has to stay a C header -- and prints sizeof of each struct and
    offsetof / size of each of its fields: the oracle of the header reader, independent of it)."""
    import subprocess
    from selfreconcode_amd import _lib
    pairs = {"sr_tensor5": _lib.SrTensor5, "sr_gemm_args": _lib.SrGemmArgs, "sr_gemm_tn_args": _lib.SrGemmTnArgs, "sr_gemm_tn_group_args": _lib.SrGemmTnGroupArgs, "sr_lbs_args": _lib.SrLbsArgs,
             "sr_newton_args": _lib.SrNewtonArgs, "sr_newton2_args": _lib.SrNewton2Args, "sr_chain_args": _lib.SrChainArgs,
             "sr_refine_args": _lib.SrRefineArgs, "sr_pack_layer": _lib.SrPackLayer, "sr_pack_table": _lib.SrPackTable,
             "sr_unpack_layer": _lib.SrUnpackLayer, "sr_unpack_table": _lib.SrUnpackTable, "sr_camera": _lib.SrCamera,
             "sr_ray_pixels": _lib.SrRayPixels, "sr_adam_tensor": _lib.SrAdamTensor, "sr_adam_table": _lib.SrAdamTable,
             "sr_frame_ids": _lib.SrFrameIds, "sr_log_slots": _lib.SrLogSlots}
    bodies = _struct_bodies()
    declared = set(bodies)
    assert len(pairs) == 19 and declared == set(pairs), declared ^ set(pairs)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "selfrecon_hip.h"\nint main(void){\n'
                   + "".join(f'printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs)
                   + "".join(f'printf("{n}.{f} %zu %zu\\n", offsetof({n}, {f}), sizeof((({n}*)0)->{f}));\n' for n, cls in pairs.items() for f, _ in cls._fields_)
                   + "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in out.strip().splitlines()}
    nfields = 0
    for n, cls in pairs.items():
        assert rows[n] == [ctypes.sizeof(cls)], (n, rows[n], ctypes.sizeof(cls))
        names = re.findall(r"(\w+)\s*(?:\[\w+\]\s*)*[,;]", bodies[n])
        assert names == [f for f, _ in cls._fields_], (n, names)                  # the class has every field of the C struct, in order
        for f, off, size in _flat_fields(cls):
            assert rows[f"{n}.{f}"] == [off, size], (n, f, rows[f"{n}.{f}"], off, size)
            nfields += 1
    assert nfields == len(rows) - len(pairs) > 150


def test_python_mirrors_of_the_header_constants():
    """Constants bound what the wrappers accept or allocate and size the by-value tables: every integer #define of the header is an
    attribute of _lib with its value (by this file's own reading of the header, not the package's), every name an operator module
    keeps for one equals it, and the error codes _lib names are the header's."""
    from selfreconcode_amd import _lib, align, mesh_prep_ops, mlp_engine, ops, step_ops, video_ops
    d = _defines()
    assert d["SR_OK"] == 0 and d["SR_STEP_LOSS_SLOTS"] == 1 + 2 * d["SR_STEP_MAX_FRAMES"]          # (the parser follows a #define that uses another)
    txt = open(os.path.join(ROOT, "include", "selfrecon_hip.h")).read()
    assert len(d) == 36 and set(d) == set(re.findall(r"^[ \t]*#define[ \t]+(SR_\w+)", txt, flags=re.M))         # every SR_* define is an integer one
    for name, value in d.items():
        assert getattr(_lib, name) == value and type(getattr(_lib, name)) is int, (name, value, getattr(_lib, name))
    assert {k for k in vars(_lib) if k.startswith("SR_")} == set(d)
    mirrors = {"SR_LBSW_MAX_K": ops.LBSW_MAX_K, "SR_SMPL_BATCH_TILE": ops.SMPL_BATCH_TILE, "SR_MESHREG_LAP": ops.MESHREG_LAP,
               "SR_MESHREG_EDGE": ops.MESHREG_EDGE, "SR_MESHREG_NORMAL": ops.MESHREG_NORMAL, "SR_EDT_EMPTY": ops.EDT_EMPTY,
               "SR_FRAMES_MAX_BATCH": ops.FRAMES_MAX_BATCH, "SR_LOG_MAX_SLOTS": ops.LOG_MAX_SLOTS,
               "SR_ACT_NONE": mlp_engine.ACT_NONE, "SR_ACT_SOFTPLUS100": mlp_engine.ACT_SOFTPLUS100, "SR_ACT_RELU": mlp_engine.ACT_RELU,
               "SR_EPI_FWD": mlp_engine.EPI_FWD, "SR_EPI_BWD": mlp_engine.EPI_BWD,
               "SR_ICP_MAX_BLOCKS": align.MAX_BLOCKS, "SR_ICP_COLS": align.COLS, "SR_ICP_HISTORY": align.HISTORY, "SR_ICP_STATE": align.STATE,
               "SR_ICP_DONE": align.DONE, "SR_QUADRIC_CLAMPED": mesh_prep_ops.QUADRIC_CLAMPED, "SR_QUADRIC_NO_PLANES": mesh_prep_ops.QUADRIC_NO_PLANES,
               "SR_STEP_MAX_FRAMES": step_ops.MAX_FRAMES, "SR_STEP_LOSS_SLOTS": step_ops._SLOTS, "SR_JPEG_BLOCK_BYTES": video_ops.BLOCK_BYTES}
    for name, value in mirrors.items():
        assert d[name] == value, (name, d[name], value)
    assert step_ops.MAX_FRAMES == d["SR_STEP_MAX_FRAMES"]
    codes = {d[n]: n for n in ("SR_EINVAL", "SR_ELAUNCH", "SR_ENOSPC")}
    assert set(codes) == set(_lib._CODES)
    for value, name in codes.items():
        assert _lib._CODES[value].startswith(name + " "), (value, _lib._CODES[value])


def test_signature_spot_table():
    """Restype and argtypes of a hand-written sample of prototypes in which every type word and form of the header occurs: struct by
    value, const struct*, double, uint32_t, float, int, int32_t, int64_t, uint8_t*, const void*, host_ arrays, the int64_t and the
    const char* returns, prototypes that span lines with a /*nullable*/ comment inside."""
    from selfreconcode_amd import _lib
    c = ctypes
    vp, i32, i64, f32, f64, T5 = c.c_void_p, c.c_int32, c.c_int64, c.c_float, c.c_double, _lib.SrTensor5
    table = {
        "sr_gridsample3d_dbwd_f16": (c.c_int, [vp, T5, vp, T5, vp, T5, vp, T5, vp, T5, vp, T5, vp, vp, vp]),
        "sr_gridsample3d_bwd_f32": (c.c_int, [vp, T5, vp, T5, vp, T5, vp, T5, vp, vp]),
        "sr_mc_emit": (c.c_int, [vp, i32, i32, i32, f32, vp, f32, f32, f32, f32, f32, f32, vp, vp, vp]),
        "sr_mc_workspace_bytes": (i64, [i32, i32, i32]),
        "sr_icp_solve": (c.c_int, [vp, i32, f64, f64, f64, f64, i32, f64, i32, i32, vp, vp, vp]),
        "sr_stream_flag_set": (c.c_int, [vp, c.c_uint32, vp]),
        "sr_stream_flag_wait": (c.c_int, [vp, c.c_uint32, vp, i32, vp]),
        "sr_lbs_chain_fwd": (c.c_int, [vp, i32, vp, vp, vp, vp, vp, vp]),
        "sr_mlp_gemm_tn_workspace_floats": (i64, [i32, i32, i64, vp]),
        "sr_mlp_gemm_nt": (c.c_int, [vp, vp]),
        "sr_mask_iou_loss_fwd": (c.c_int, [vp, vp, c.c_int, i64, vp, vp, vp]),
        "sr_minv3x3_fwd_f64": (c.c_int, [vp, vp, vp, i64, vp]),
        "sr_pe_embed": (c.c_int, [vp, i64, i32, vp, vp, i64, i32, vp, i32, vp, i64, vp]),
        "sr_step_reduce_blocks": (c.c_int, [i64]),
        "sr_log_row": (c.c_int, [vp, i32, vp, i32, i32, i64, vp]),
        "sr_frames_fetch": (c.c_int, [vp, vp, vp, i64, i64, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp]),
        "sr_build_digest": (c.c_char_p, []),
        "sr_abi_version": (c.c_int, []),
    }
    for name, (restype, argtypes) in table.items():
        f = getattr(_lib._lib, name)
        assert f.restype is restype, (name, f.restype)
        assert list(f.argtypes or []) == argtypes, (name, f.argtypes)
        if not name.startswith(("sr_build", "sr_abi")):
            assert _lib.SIGNATURES[name] == argtypes and _lib.raw(name) is f, name
    # what the table's rows stand for, over all 151: the int64_t returns are the size functions, every entry point that launches takes the stream last
    assert len(_lib.SIGNATURES) == 148
    wide = {n for n in _lib.SIGNATURES if _lib.raw(n).restype is i64}
    assert wide == {n for n in _lib.SIGNATURES if n.endswith(("_workspace_floats", "_workspace_bytes"))} and len(wide) == 10
    assert all(_lib.raw(n).restype is c.c_int for n in set(_lib.SIGNATURES) - wide)


@pytest.mark.parametrize("text, names", [
    ("int sr_f(const foo_t* x, void* stream);", "foo_t"),                                             # unknown type word behind a pointer
    ("int sr_f(unsigned x);", "unsigned"),                                                            # ... by value
    ("long sr_f(void);", "long"),                                                                     # ... as a return type
    ("typedef struct { size_t n; } sr_s;", "size_t"),                                                 # ... in a field
    ("typedef struct { int32_t id[SR_MISSING]; } sr_s;", "SR_MISSING"),                               # undefined array dimension
    ("#define SR_N 4\nint sr_f(void* stream);\nint sr_f(int64_t n, void* stream);", "sr_f"),          # duplicate function
    ("#define SR_N 4\n#define SR_N 5\n", "SR_N"),                                                     # duplicate define
    ("typedef struct { int a; } sr_s;\ntypedef struct { int b; } sr_s;", "sr_s"),                     # duplicate struct
    ("#define SR_N (1 +\n", "SR_N"),                                                                  # malformed defines
    ("#define SR_N 4u\n", "SR_N"),
    ("#define SR_N SR_LATER\n#define SR_LATER 1\n", "SR_N"),
    ("#define SR_N\n", "SR_N"),
    ("int sr_f(int64_t, void* stream);", "int64_t"),                                                  # unparsable declarators
    ("int sr_f(float (*cb)(int), void* stream);", "cb"),
    ("typedef struct { float* a, b; } sr_s;", "float* a, b"),
    ("int sr_f(void* stream)", "sr_f"),                                                               # no terminating ;
    ("typedef struct sr_t_s sr_t;", "sr_t_s"),                                                        # typedef of an undeclared struct
    ("#pragma pack(1)\n", "pragma"),
])
def test_header_reader_refuses_what_it_does_not_understand(text, names):
    from selfreconcode_amd import _abi
    with pytest.raises(_abi.AbiError, match=re.escape(names)):
        _abi.parse(text)


def test_header_reader_on_a_small_header():
    from selfreconcode_amd import _abi
    c = ctypes
    d, s, f = _abi.parse("/* c */\n#ifndef G_\n#define G_\n#include <stdint.h>\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n#define SR_N (1 + 2)   /* n */\n"
                         "typedef struct { const float* p[2]; uint8_t k[SR_N], j; double d; } sr_s;\n"
                         "struct sr_t_s {\n  sr_s s[2][SR_N];\n};\ntypedef struct sr_t_s sr_t;\n"
                         "int64_t sr_f(const sr_t* host_t, sr_s v /*nullable*/,\n             double x, void* stream);\nconst char* sr_g(void);\n"
                         "#ifdef __cplusplus\n}\n#endif\n#endif\n")
    assert d == {"SR_N": 3} and list(s) == ["sr_s", "sr_t"] and s["sr_s"].__name__ == "SrS"
    assert _flat_fields(s["sr_s"]) == [("p", 0, 16), ("k", 16, 3), ("j", 19, 1), ("d", 24, 8)] and c.sizeof(s["sr_t"]) == 6 * 32
    assert s["sr_t"]._fields_[0][1] is (s["sr_s"] * 3) * 2
    assert f == {"sr_f": (c.c_int64, [c.c_void_p, s["sr_s"], c.c_double, c.c_void_p]), "sr_g": (c.c_char_p, [])}


def test_header_reader_imports_without_torch_or_the_library():
    import subprocess
    import sys
    code = ("import sys; from selfreconcode_amd import _abi; d, s, f = _abi.load(); "
            "assert len(d) == 36 and len(s) == 19 and len(f) == 151, (len(d), len(s), len(f)); "
            "bad = [m for m in ('torch', 'numpy', 'selfreconcode_amd._lib', 'selfreconcode_amd.build') if m in sys.modules]; assert not bad, bad")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_pack_cache_entries_die_with_their_parameters():
    """mlp_engine keeps packed weights / gradient buffers per parameter; the entry must not outlive (or keep alive) the module."""
    import gc
    import torch
    from selfreconcode_amd import mlp_engine as me

    lin = torch.nn.Linear(8, 4)
    key = id(lin.weight)
    W = torch.zeros(4, 8)                                 # (a CPU tensor: the registry needs no GPU)
    e = me._pack_entry(key, ("sig",), lambda: me._Pack(W, W.t().contiguous(), None), owner=lin.weight)
    assert me._PACK_CACHE[key] is e and me._ENTRY_BY_PTR[W.data_ptr()] is e
    import weakref
    e.src = (weakref.ref(lin.weight),)
    del lin
    gc.collect()
    assert key not in me._PACK_CACHE and W.data_ptr() not in me._ENTRY_BY_PTR
    for name, reg in vars(me).items():                    # no registry of the engine holds the entry or the pointer
        if isinstance(reg, (dict, set)) and not name.startswith("__"):
            held = list(reg) + (list(reg.values()) if isinstance(reg, dict) else [])
            assert not any(x is e or (isinstance(x, int) and x == W.data_ptr()) for x in held), name
