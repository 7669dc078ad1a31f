"""include/ms2_plugin_abi.h restates the slice of mediastreamer2's plugin ABI the facades use (the real headers need
bctoolbox / oRTP, absent from the image, so -DMSMI355X_USE_REAL_MS2_HEADERS cannot be compiled here).  What CAN be
checked mechanically is checked here: the reference's headers (include/mediastreamer2/) are PARSED, never copied, by
reference_facts() below, and every id, method macro, enum value and struct field list our header declares is compared
with what they say.  What they say about those names is stored in tests/golden/ms2_abi.json
(tests/golden/make_abi_golden.py <reference tree> regenerates it), so the comparison runs wherever the suite does."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OURS = os.path.join(ROOT, "include", "ms2_plugin_abi.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ms2_abi.json")


def strip_comments(txt):
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    return re.sub(r"\\\n", " ", txt)  # continuation lines joined


def ours():
    txt = strip_comments(open(OURS).read())
    return txt[txt.index("#else"):]  # the restated part, not the real-headers include list


def enum_values(txt, opener):
    """{name: value} of the enum whose text starts at `opener`, counting implicit values like the compiler"""
    m = re.search(opener + r"\s*\{(.*?)\}", txt, flags=re.S)
    assert m, opener
    out, nxt = {}, 0
    for item in m.group(1).split(","):
        item = item.strip()
        if not item:
            continue
        if "=" in item:
            name, expr = [x.strip() for x in item.split("=", 1)]
            expr = re.sub(r"(\d+)u\b", r"\1", expr)
            nxt = int(eval(expr, {"__builtins__": {}}, dict(out)))  # noqa: S307 -- header constants: integers, +, <<
        else:
            name = item
        out[name] = nxt
        nxt += 1
    return out


def method_defines(txt):
    """{NAME: (macro, args...)} for every #define NAME MS_FILTER_*(...) line; whitespace-normalised arguments"""
    out = {}
    for m in re.finditer(r"#define\s+(\w+)\s+(MS_FILTER_(?:BASE_)?(?:METHOD|EVENT)(?:_NO_ARG)?)\s*\(([^)]*)\)", txt):
        args = tuple(re.sub(r"\s+", " ", a.strip()) for a in m.group(3).split(","))
        out[m.group(1)] = (m.group(2),) + args
    return out


def struct_fields(txt, opener):
    """the declarators of a struct body in order, normalised: 'type name' with pointer stars attached to the name"""
    m = re.search(opener + r"\s*\{", txt)
    assert m, opener
    i, depth, body = m.end(), 1, []
    while depth:
        c = txt[i]
        depth += (c == "{") - (c == "}")
        body.append(c)
        i += 1
    body = "".join(body[:-1])
    body = re.sub(r"#else.*?#endif", " ", body, flags=re.S)  # the 64-bit branch of a pointer-size #if (this target)
    body = re.sub(r"#[^\n]*", " ", body)
    body = re.sub(r"\{[^{}]*\}", "{}", body)  # nested union / struct bodies compared separately
    fields = []
    for decl in body.split(";"):
        decl = re.sub(r"\s+", " ", decl).strip()
        if decl:
            fields.append(re.sub(r"\(\s+", "(", re.sub(r"\s*\*\s*", " *", decl)))
    return fields


STRUCTS = [
    ("msfilter.h", r"struct _MSFilterMethod"),
    ("msfilter.h", r"struct _MSFilterDesc"),
    ("msaudiomixer.h", r"typedef struct MSAudioMixerCtl"),
    ("msequalizer.h", r"typedef struct _MSEqualizerGain"),
    ("flowcontrol.h", r"typedef struct _MSAudioFlowControlDropEvent"),
    ("flowcontrol.h", r"typedef struct _MSAudioFlowControlConfig"),
    ("msvideo.h", r"typedef struct _MSPicture"),
    ("msvideo.h", r"struct _MSScalerDesc"),
    ("msqueue.h", r"typedef struct _MSCPoint"),
    ("msqueue.h", r"typedef struct _MSQueue"),
    ("msqueue.h", r"struct _MSBufferizer"),
]
METHOD_HEADERS = ("msfilter.h", "msvolume.h", "msaudiomixer.h", "msequalizer.h", "msinterfaces.h", "flowcontrol.h",
                  "mschanadapter.h", "msgenericplc.h", "msvideo.h")
METHOD_ID = r"#define\s+MS_FILTER_METHOD_ID\s*\(_id_,\s*_cnt_,\s*_argsize_\)([^\n]*)\n"


def norm(s):
    return re.sub(r"\s+", "", s)


def field_names(fields):
    return [re.split(r"[ *]", f)[-1].split("[")[0] for f in fields]


def flat(v):
    return [y.strip() for x in v for y in x.split(",")]


def our_enums():
    """{enum: {name: value}} of the enums our header restates"""
    mine = ours()
    return {"MSFilterId": enum_values(mine, r"typedef enum MSFilterId"),
            "MSFilterInterfaceId": enum_values(re.search(r"enum\s*\{\s*MSFilterInterfaceBegin.*?\}", mine, flags=re.S).group(0), r"enum"),
            "MSFilterCategory": enum_values(mine, r"enum _MSFilterCategory"),
            "MSFilterFlags": enum_values(mine, r"enum _MSFilterFlags"),
            "MSPixFmt": enum_values(mine[mine.index("MS_PIX_FMT_UNKNOWN") - 40:], r"typedef enum"),
            "MSVideoOrientation": enum_values(mine, r"typedef enum MSVideoOrientation")}


def reference_facts(read_ref):
    """What the reference's headers say about every name our header declares: the other side of each comparison below.
    read_ref(*header names) -> the text of those headers of include/mediastreamer2/, comments stripped.  Only the names
    ms2_plugin_abi.h itself restates are kept."""
    mine = ours()
    ref = read_ref("msfilter.h", "msvideo.h")
    pix = enum_values(ref, r"typedef enum _MSPixFmt") if re.search(r"typedef enum _MSPixFmt", ref) else enum_values(
        ref[ref.index("MS_PIX_FMT_UNKNOWN") - 40:], r"typedef enum\s*\w*")
    enums = {"MSFilterId": enum_values(read_ref("allfilters.h"), r"typedef enum MSFilterId"),
             "MSFilterInterfaceId": enum_values(read_ref("msfilter.h"), r"enum _MSFilterInterfaceId"),
             "MSFilterCategory": enum_values(ref, r"enum _MSFilterCategory"),
             "MSFilterFlags": enum_values(ref, r"enum _MSFilterFlags"),
             "MSPixFmt": pix,
             "MSVideoOrientation": enum_values(ref, r"typedef enum MSVideoOrientation")}
    enums = {e: {k: v for k, v in enums[e].items() if k in names} for e, names in our_enums().items()}
    methods = method_defines(read_ref(*METHOD_HEADERS))
    n_filter = len(flat(field_names(struct_fields(mine, r"typedef struct _MSFilter"))))
    ticker = field_names(struct_fields(mine, r"typedef struct _MSTicker"))
    return {
        "enums": enums,
        "methods": {k: v for k, v in methods.items() if k in method_defines(mine)},
        "method_id_macro": norm(re.search(METHOD_ID, read_ref("msfilter.h")).group(1)),
        "structs": {opener: struct_fields(read_ref(header), opener) for header, opener in STRUCTS},
        "MSFilter_prefix": flat(field_names(struct_fields(read_ref("msfilter.h"), r"struct _MSFilter")))[:n_filter],
        "MSTicker_prefix": field_names(struct_fields(read_ref("msticker.h"), r"struct _MSTicker"))[:ticker.index("time") + 1],
    }


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_filter_ids_match_allfilters_h(golden):
    ref = golden["enums"]["MSFilterId"]
    mine = our_enums()["MSFilterId"]
    assert len(mine) >= 20
    for name, val in mine.items():
        assert name in ref, name
        assert ref[name] == val, f"{name}: ms2_plugin_abi.h says {val}, allfilters.h counts {ref[name]}"


def test_interface_ids_match_msfilter_h(golden):
    ref = golden["enums"]["MSFilterInterfaceId"]
    for name, val in our_enums()["MSFilterInterfaceId"].items():
        assert ref[name] == val, (name, val, ref[name])


def test_category_flags_and_pixfmt_enums(golden):
    mine = our_enums()
    for enum in ("MSFilterCategory", "MSFilterFlags", "MSPixFmt", "MSVideoOrientation"):
        r = golden["enums"][enum]
        for name, val in mine[enum].items():
            assert r[name] == val, (name, val, r[name])


def test_method_and_event_macros_match(golden):
    ref = {k: tuple(v) for k, v in golden["methods"].items()}
    mine = method_defines(ours())
    assert len(mine) >= 60, len(mine)
    missing = [n for n in mine if n not in ref]
    # macro helpers our header defines in terms of each other (not ids) are not in the reference under that shape
    assert not missing, missing
    for name, spec in mine.items():
        assert ref[name] == spec, f"{name}: ours {spec}, reference {ref[name]}"


def test_the_method_id_packing_macro(golden):
    b = re.search(METHOD_ID, ours() + "\n")
    assert b
    assert golden["method_id_macro"] == norm(b.group(1))


@pytest.mark.parametrize("header,opener", STRUCTS)
def test_struct_field_lists_match(golden, header, opener):
    a = golden["structs"][opener]
    b = struct_fields(ours(), opener)
    canon = lambda f: re.sub(r"\bstruct _MSFilter\b", "MSFilter", re.sub(r"\bstruct (_\w+)\b", r"struct \1", f))  # noqa: E731
    assert [canon(x) for x in a] == [canon(x) for x in b], (a, b)


def test_filter_and_ticker_layout_prefixes(golden):
    """MSFilter up to `seen` and MSTicker up to `time`: the same fields in the same order (types modulo the ms_mutex_t =
    pthread_mutex_t / MSList = bctbx_list_t aliases of ortp/port.h, which our header spells out)."""
    b = field_names(struct_fields(ours(), r"typedef struct _MSFilter"))
    assert golden["MSFilter_prefix"] == flat(b), (golden["MSFilter_prefix"], b)
    b = field_names(struct_fields(ours(), r"typedef struct _MSTicker"))
    upto = b.index("time") + 1
    assert golden["MSTicker_prefix"] == b[:upto], (golden["MSTicker_prefix"], b)
