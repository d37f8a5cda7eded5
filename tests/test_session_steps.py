"""Which steps a device-resident session plans (source/mi355x_opt/session.c:plan_fusion), pinned as text.
shl_mi355x_session_describe writes one line per step -- the rule's name ("layer" for a plain one), the layers it stands for,
the tensor it writes, an attention step's four fold counts and whether it carries a bias -- and the folded-activation count.
The graphs are the ones the session tests of every fusion build, each under the default environment, under
SHL_MI355X_NO_FUSION=1 and under its family's own switches at 0 and at 1; sessions are set up (which captures them) and not run.

The literals in tests/golden/session_steps.json were dumped from the library built at the commit before the planner's rule
table replaced enum step_kind, merged_kind and the inline attention block, by the same describe function written against the
old struct step, on an MI355X; they are not derived from the rule table."""
import contextlib
import ctypes as C
import importlib
import json
import os

import pytest

import act_fuse_cases as ac
import dw_act_cases as dc
import linear_cases as lc
import residual_f16_nets as fn
import residual_nets as rn
import test_attention_bias_session as tb
import test_attention_layout_session as tl
import test_session_plan as tp
from cases import pkg
from test_attention_session import attention_net

wl = importlib.import_module("csi-nn2_amd.workloads")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "session_steps.json")
ATT, LAY, RES, ACT, FORM = ("SHL_MI355X_ATTENTION", "SHL_MI355X_ATTENTION_LAYOUT", "SHL_MI355X_RESIDUAL", "SHL_MI355X_ACT_FUSE",
                            "SHL_MI355X_MATMUL_FORM")
CLEARED = (ATT, LAY, RES, ACT, FORM, "SHL_MI355X_NO_FUSION", "SHL_MI355X_HOST_SESSION", "SHL_MI355X_ADD_FORM", "SHL_MI355X_MUL_FORM",
           "SHL_MI355X_TRANSPOSE_FORM", "SHL_MI355X_ACT_FORM", "SHL_MI355X_RESIDUAL_FORM", "SHL_MI355X_IGEMM", "SHL_MI355X_PWDW",
           "SHL_MI355X_DWMFMA")

BOTH = [{}, {"SHL_MI355X_NO_FUSION": "1"}]
SWITCHED = {"plain": [],
            "residual": [{RES: "0"}, {RES: "1"}],
            "act": [{ACT: "0"}, {ACT: "1"}],
            "attention": [{ATT: "0"}, {ATT: "1"}, {ATT: "1", LAY: "0"}, {ATT: "1", LAY: "1"}, {LAY: "0"}, {LAY: "1"}]}


class _Model:
    """workloads.ModelSession under the nets' build / close"""

    def __init__(self, batch):
        self.batch = batch

    def build(self, fe, api):
        self.ms = wl.ModelSession(fe, api, "int8", "NHWC", batch=self.batch)
        return self.ms.sess

    def close(self, fe):
        self.ms.close()


def _graphs():
    """name -> (family, environment every build of it has, constructor)"""
    g = {}
    for make in (tp.pair_with_both_halves_folded, tp.two_consumers, tp.fold_in_front_of_conv_pool):
        g["plan/" + make.__name__] = ("plain", {}, make)
    for name in ("basic_block", "inverted_block", "projection_block", "broadcast_block"):
        g["residual/" + name] = ("residual", {}, getattr(rn, name))
    for name in ("basic_block", "inverted_block", "projection_block", "broadcast_block", "bottleneck_tail"):
        g["residual_f16/" + name] = ("residual", {}, getattr(fn, name))
    for mod, tag in ((ac, "act/"), (dc, "dw_act/")):
        for name, entry in mod.FUSING.items():
            g[tag + name] = ("act", {}, entry[0])
        for name, make in mod.APART.items():
            g[tag + name] = ("act", {}, make)
    g["attention/block"] = ("attention", {}, lambda: attention_net("int8", "NHWC"))
    g["attention/block_f16"] = ("attention", {}, lambda: attention_net("f16", "NCHW"))
    g["attention/second_consumer"] = ("attention", {}, lambda: attention_net("int8", "NHWC", second_consumer=True))
    g["attention/p_is_output"] = ("attention", {}, lambda: attention_net("int8", "NHWC", p_is_output=True))
    for name, (make, form) in tb.NETS.items():
        g["attention_bias/" + name] = ("attention", {FORM: form} if form else {}, lambda make=make: make("int8", "NHWC"))
    for make in (tl._qh_read_twice, tl._k_requantised, tl._q_inner_swapped, tl._k_as_onnx):
        g["attention_layout/" + make.__name__.lstrip("_")] = ("attention", {}, lambda make=make: make("int8", "NHWC"))
    # Swin windows at batch 16: unset, the dense default leaves the core apart and the eight moves bring it in
    g["attention_layout/promoted"] = ("attention", {}, lambda: tb.block("int8", "NHWC", 16, 49, 3, 32, (16, 1, 1, 49), mask=True))
    for name, make in lc.NETS.items():
        g["linear/" + name] = ("plain", {}, lambda make=make: make("int8", "NHWC"))
    g["mobilenetv1/batch1"] = ("plain", {}, lambda: _Model(1))
    g["mobilenetv1/batch128"] = ("plain", {}, lambda: _Model(128))
    return g


GRAPHS = _graphs()


def env_key(env):
    return " ".join("%s=%s" % (k.replace("SHL_MI355X_", ""), v) for k, v in sorted(env.items())) or "default"


@contextlib.contextmanager
def environment(env):
    """the planner's switches cleared, then `env`; restored afterwards (they are read at setup)"""
    saved = {k: os.environ.pop(k, None) for k in CLEARED}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in CLEARED:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def describe(opt, sess):
    fn_ = opt.shl_mi355x_session_describe
    fn_.restype, fn_.argtypes = C.c_int, [C.c_void_p, C.c_char_p, C.c_int]
    need = fn_(sess, None, 0)
    buf = C.create_string_buffer(max(need, 1))
    assert fn_(sess, buf, need) == need
    return buf.value.decode()


def plans(fe, opt, name):
    """environment key -> the described plan of graph `name` built under it"""
    family, base, make = GRAPHS[name]
    res = {}
    for env in BOTH + SWITCHED[family]:
        with environment(dict(base, **env)):
            net = make()
            sess = net.build(fe, pkg.API_MI355X)
            assert opt.shl_mi355x_session_is_device_resident(sess) == 2, "the session is not one captured hipGraph"
            res[env_key(env)] = describe(opt, sess)
            net.close(fe)
    return res


@pytest.fixture(scope="module")
def gpu():
    fe = pkg.load_frontend("standalone")
    hip, opt = pkg.load_backend(fe)
    if hip.shl_mi355x_device_count() < 1:
        pytest.fail("no gfx950 device visible: " + hip.shl_mi355x_last_error().decode())
    return fe, hip, opt


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_graph_and_environment_has_a_recorded_plan(recorded):
    assert sorted(recorded) == sorted(GRAPHS)
    for name, (family, _, _) in GRAPHS.items():
        assert sorted(recorded[name]) == sorted(env_key(e) for e in BOTH + SWITCHED[family]), name
        assert all(text.endswith("\n") and text.splitlines()[-1].startswith("folded ") for text in recorded[name].values()), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_the_session_plans_the_recorded_steps(gpu, recorded, name):
    fe, hip, opt = gpu
    got = plans(fe, opt, name)
    for key in sorted(got):
        print("%s [%s]\n%s" % (name, key, got[key]))
    for key in sorted(got):
        assert got[key] == recorded[name][key], "%s under %s plans other steps than the parent did" % (name, key)
