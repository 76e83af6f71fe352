"""The code that opens and closes an AR step, stand-alone and value by value on host operands (ptts_debug_step_edge): k_step_begin, k_step_begin_mm, k_step_finish
(csrc/kernels.hip) and the two last-launch instances of the step linear, k_skinny<WT, false, PRO_LN | PRO_MOD, 2, 4, FIN> and <..., FIN, CHAIN> (csrc/skinny.hip),
which produce every frame the product emits -- the second one the next step's x, fx and x0 as well.

What they replace: the tail of the generation loop (internal/tts/runtime_native_safetensors.go:176-192 and the loop's bound :155; the strict EOS comparison
flow_lm.go:281), the step's input (the previous frame, NaN -> bos: :246-253, tensor_util.go:259-268; input_linear flow_lm.go:254; input_proj flow_net.go:327)
and flowFinalLayer.Forward with the Euler update (flow_net.go:205-239, flow_lm.go:311-353).  The reference side is tests/_step_edge_ref.py.

Every id names the form reached, and every call's census is asserted to show that kernel.  Rows: B in {1, 5, 15, 16, 17, 33, 256} -- the row-tile edges of
k_skinny (16 rows per tile, 4 per lane group), the 16-row blocks of k_step_begin_mm, the full 16-tile grid whose blocks all hit n_active.  Every operand holds
PAD more rows than are launched: those must come back as they went.  The state is a crafted table (TABLE) so that each rule of the books is met by a row made
for it, whatever a checkpoint's logits would do.

Tolerances are the project's existing ones, none is new: the books, the frame's place, in32 and x0 are exact; x and fx are held to 3e-5 * (sum |w v| + |b|) +
1e-6 and the frame to the AXPY form of that bound (tests/test_gpu_step_linear.py: TOL, FLOOR, its alpha factor; tests/test_gpu_tall.py).
test_emulation_stays_within_half_the_bound (no GPU) holds a numpy emulation of so_tile to half of it; test_planted_defects_are_caught (no GPU) shows that the
checks tell six wrong readings of the rules from the right one."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _step_edge_ref as R
import test_gpu_step_linear as SL
from _kernel_ref import bf16_bits, bf16_round, bits, check_bound, untouched

TOL, FLOOR = SL.TOL, SL.FLOOR
F32 = np.float32
gpu = pytest.mark.gpu
S = 6            # frames a row's latents hold
PAD = 2          # rows held behind the B that are launched
LIST_B = [1, 5, 15, 16, 17, 33, 256]
WF = SL.WF
ALPHA, EPS = 0.25, 1e-6
WIDTHS = [(16, 16), (1024, 512), (1040, 528), (2064, 1040)]   # (d_in, d_pj): the c_n - 16 / N - 4 clamps; the model's; two that run the chained tail's second and third pass
NAN, INF = float("nan"), float("inf")

# one row per rule of the books (defaults: active, max_steps 6, no countdown, frames_after_eos 1, threshold 0, logit -1: no EOS, kv_len = step + 5)
TABLE = [
    dict(name="inactive", active=0, step=3, logit=5.0),
    dict(name="EOS, frames_after_eos 0", step=2, fae=0, thr=0.5, logit=0.75),
    dict(name="EOS, frames_after_eos 2", step=1, fae=2, thr=-1.0, logit=0.0),
    dict(name="logit == threshold", step=2, fae=0, thr=0.25, logit=0.25),
    dict(name="NaN logit", step=1, fae=0, logit=NAN),
    dict(name="threshold +inf", step=3, fae=0, thr=INF, logit=3e38),
    dict(name="countdown 0 already", step=3, cd=0, fae=2, eos_step=1),
    dict(name="countdown 3, EOS again", step=2, cd=3, fae=5, eos_step=1, logit=1.0),
    dict(name="last step, no EOS", step=3, max=4),
    dict(name="last step and countdown 0", step=4, max=5, cd=0, eos_step=2),
    dict(name="step 0", step=0),
    dict(name="NaNs in the previous frame", step=2, nan_prev=True),
    dict(name="kv_len != step", step=1, kv=17),
]
ROW0 = dict(active=1, step=1, max=S, cd=-1, fae=1, thr=0.0, logit=-1.0, eos_step=-1, kv=None, nan_prev=False)


def table_rows(B, rot, rng):
    """B row specs: all of TABLE at scattered places and random rows between them (B >= 17), else the B entries of TABLE from `rot` on."""
    if B < len(TABLE) + 4:
        return [dict(ROW0, **TABLE[(rot + i) % len(TABLE)]) for i in range(B)]
    rows = []
    for _ in range(B):
        st = int(rng.integers(0, 5))
        rows.append(dict(ROW0, active=int(rng.random() < 0.8), step=st, max=int(rng.integers(st + 1, S + 1)), cd=int(rng.choice([-1, -1, -1, 0, 2])),
                         fae=int(rng.integers(0, 3)), logit=float(rng.standard_normal())))
    for spec, at in zip(TABLE, rng.permutation(B)[:len(TABLE)]):
        rows[int(at)] = dict(ROW0, **spec)
    return rows


def make_case(B, seed, *, ldim=32, rot=0, noise=True):
    """state, latents, noise, bos, logits and a frame for B launched rows (+ PAD behind them).  Latents: random frames below `step`, 0xff bytes from there on."""
    rng = np.random.default_rng(zlib.crc32(f"{B}-{seed}-{ldim}-{rot}".encode()))
    specs = table_rows(B, rot, rng) + [dict(ROW0, logit=9.0, fae=0)] * PAD   # (the rows behind B would run, and end, if a kernel took them)
    rows = B + PAD
    st = {k: np.zeros(rows, np.int32) for k in R.STATE_I32}
    thr, logit = np.zeros(rows, F32), np.zeros(rows, F32)
    lat = np.full((rows, S * ldim), np.nan, F32)
    lat.view(np.uint32)[:] = 0xFFFFFFFF
    for r, sp in enumerate(specs):
        st["active"][r], st["step"][r], st["max_steps"][r], st["countdown"][r] = sp["active"], sp["step"], sp["max"], sp["cd"]
        st["frames_after_eos"][r], st["eos_step"][r], st["n_frames"][r] = sp["fae"], sp["eos_step"], sp["step"]
        st["kv_len"][r] = sp["step"] + 5 if sp["kv"] is None else sp["kv"]
        thr[r], logit[r] = sp["thr"], sp["logit"]
        lat[r, :sp["step"] * ldim] = rng.standard_normal(sp["step"] * ldim)
        if sp["nan_prev"]:
            lat[r, (sp["step"] - 1) * ldim + np.array([0, 3, ldim - 1])] = np.nan
    st["eos_threshold"], st["n_active"] = thr, int(st["active"][:B].sum())
    return dict(B=B, rows=rows, ldim=ldim, state=st, latents=lat, noise=rng.standard_normal((rows, S * ldim)).astype(F32) if noise else None,
                bos=rng.standard_normal(ldim).astype(F32), logit=logit, frame=rng.standard_normal((rows, ldim)).astype(F32), lin=None, final=None, rng=rng)


def add_lin(c, d_in, d_pj, bf16, biases):
    rng, ld = c["rng"], c["ldim"]
    w_in, w_pj = (0.2 * rng.standard_normal((d_in, ld))).astype(F32), (0.2 * rng.standard_normal((d_pj, ld))).astype(F32)
    c["lin"] = dict(w_in=bf16_bits(w_in) if bf16 else w_in, w_pj=bf16_bits(w_pj) if bf16 else w_pj,
                    b_in=rng.standard_normal(d_in).astype(F32) if biases else None, b_pj=rng.standard_normal(d_pj).astype(F32) if biases else None)
    return c


def add_final(c, K, wfmt, *, N=None, bias=True, nan_row=None):
    """the final layer's operands; nan_row: one element of that row's residual is NaN, so that one element of its frame is"""
    rng, rows = c["rng"], c["rows"]
    N = c["ldim"] if N is None else N
    cur = rng.standard_normal((rows, N)).astype(F32)
    if nan_row is not None:
        cur[nan_row, 5] = np.nan
    c["final"] = dict(fx=rng.standard_normal((rows, K)).astype(F32), W=(0.05 * rng.standard_normal((N, K))).astype(F32),
                      bias=rng.standard_normal(N).astype(F32) if bias else None, shift=(0.3 * rng.standard_normal((rows, K + 12))).astype(F32),
                      mscale=(0.3 * rng.standard_normal((rows, K + 12))).astype(F32), cur=cur, wfmt=wfmt, alpha=ALPHA, eps=EPS, epi=7)
    return c


def eff_weights(f):
    """the final linear as the kernel multiplies it"""
    return f["W"] if f["wfmt"] == 0 else (bf16_round(f["W"]) if f["wfmt"] == 1 else SL.quantize_rows(f["W"])[0])


# ------------------------------------------------------------------------------------------------ the checks (a), (b), (d): used on GPU results and, in
# test_planted_defects_are_caught, on a faultless result against a reference with a planted defect
def filled(rows, n):
    """what the hooks leave where nothing is stored: 0xff bytes"""
    return np.frombuffer(b"\xff" * (4 * rows * n), F32).reshape(rows, n)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def check_close(name, c, got, want_state, want_lat):
    """(a) every state array and n_active equal the reference's, integer for integer; what the reference does not set stays; inactive rows and the rows behind
    B stay in every array.  (b) the latents equal the reference's bit for bit: the frame at row `step` of the rows that were active, everything else as it was."""
    B, st0 = c["B"], c["state"]
    idle = np.flatnonzero(np.asarray(st0["active"][:B]) == 0)
    for k in R.STATE_I32:
        g = got["state"][k]
        assert np.array_equal(g[:B], want_state[k][:B]), (name, k, np.flatnonzero(g[:B] != want_state[k][:B])[:8], g[:B][g[:B] != want_state[k][:B]][:8])
        assert np.array_equal(g[B:], st0[k][B:]), (name, k, "rows behind B changed")
        assert np.array_equal(g[idle], st0[k][idle]), (name, k, "an inactive row changed")
    assert got["state"]["n_active"] == want_state["n_active"], (name, got["state"]["n_active"], want_state["n_active"])
    assert same_bits(got["state"]["eos_threshold"], st0["eos_threshold"]), name
    lat = got["latents"]
    bad = np.argwhere(bits(lat) != bits(want_lat))
    assert bad.size == 0, (name, "latents differ from the reference's at (row, element)", bad[:8].tolist())
    assert same_bits(lat[B:], c["latents"][B:]) and same_bits(lat[idle], c["latents"][idle]), name


def check_values(name, got, want, bound, log=True):
    if log:
        check_bound(name, got, want, bound, TOL)
    else:
        err = np.abs(np.asarray(got, np.float64) - want)
        assert np.isfinite(got).all() and float((err / bound).max()) <= 1.0, name


def check_open(name, c, got, state, latents, *, in32=True, sel=None, log=True):
    """(d) in32 and x0 bit for bit against open_() on (state, latents); x and fx against lin64 of them under the operand-split bound.  sel: the rows compared
    (default: all B).  The rows behind B of every result keep the hooks' fill."""
    B = c["B"]
    sel = np.arange(B) if sel is None else sel
    w_in32, w_x0 = R.open_(state, latents, c["noise"], c["bos"], B)
    if in32:
        assert same_bits(got["in32"][:B][sel], w_in32[sel]), (name, "in32", np.argwhere(bits(got["in32"][:B]) != bits(w_in32))[:8].tolist())
        assert untouched(got["in32"][B:]), name
    assert same_bits(got["x0"][:B][sel], w_x0[sel]), (name, "x0", np.argwhere(bits(got["x0"][:B]) != bits(w_x0))[:8].tolist())
    assert untouched(got["x0"][B:]), name
    if c["lin"] is not None and got.get("x") is not None:
        for what, v, w, b in (("x", w_in32, "w_in", "b_in"), ("fx", w_x0, "w_pj", "b_pj")):
            want, mag = R.lin64(v[sel], c["lin"][w], c["lin"][b])
            check_values(f"{name} {what}", got[what][:B][sel], want, TOL * mag + FLOOR, log)
            assert untouched(got[what][B:]), (name, what)
    return w_in32, w_x0


def run(pkg, op, c, **over):
    a = dict(c, **over)
    return pkg.runtime.debug_step_edge(op, a["state"], a["latents"], a["bos"], B=a["B"], noise=a["noise"], eos_logit=a["logit"],
                                       frame=a["frame"] if op == "finish" else None, lin=a["lin"] if op in ("begin_lin", "fin_chain") else None,
                                       final=a["final"] if op in ("fin", "fin_chain") else None)


# ------------------------------------------------------------------------------------------------ no GPU
def test_finish_restates_the_go_loop():
    """finish() driven step by step on one row collects as many frames as the Go loop written down as it stands (append, EOS arm, break or decrement), for
    random logit sequences, thresholds, frames_after_eos and max_steps -- with logits exactly at the threshold, NaN logits and a threshold of +inf among them."""
    rng = np.random.default_rng(1)
    for _ in range(3000):
        max_steps, fae = int(rng.integers(1, 12)), int(rng.integers(0, 4))
        thr = float(rng.choice([0.0, 0.5, INF]))
        logits = rng.choice([-1.0, 0.0, 0.5, 0.75, NAN], size=max_steps, p=[0.45, 0.2, 0.15, 0.1, 0.1]).astype(F32)
        st = {k: np.zeros(1, np.int32) for k in R.STATE_I32}
        st["active"][0], st["countdown"][0], st["eos_step"][0], st["max_steps"][0], st["frames_after_eos"][0] = 1, -1, -1, max_steps, fae
        st["eos_threshold"], st["n_active"] = np.array([thr], F32), 1
        calls = 0
        while st["active"][0]:
            st = R.finish(st, logits[int(st["step"][0]):], 1)
            calls += 1
            assert calls <= max_steps
        want, broke, eos_step = R.go_loop_frames(logits, thr, fae, max_steps)
        assert st["n_frames"][0] == want == calls and st["n_active"] == 0 and st["kv_len"][0] == calls, (logits, thr, fae, max_steps)
        assert st["broke"][0] == broke and st["eos_step"][0] == eos_step, (logits, thr, fae, max_steps)


def _open_cases():
    for i, (d_in, d_pj) in enumerate(WIDTHS):
        for biases in (True, False):
            for bf16 in (False, True):
                yield d_in, d_pj, biases, bf16, LIST_B[(2 * i + biases + 3 * bf16) % len(LIST_B)]


def test_emulation_stays_within_half_the_bound():
    """so_tile's arithmetic, emulated in numpy (emulate_mm), stays within HALF the bound that x and fx are held to, for every width and weight type of this file:
    the bound has room for a correct kernel."""
    worst = 0.0
    for d_in, d_pj, biases, bf16, B in _open_cases():
        c = add_lin(make_case(min(B, 33), "emu", rot=10), d_in, d_pj, bf16, biases)
        in32, x0 = R.open_(c["state"], c["latents"], c["noise"], c["bos"], c["B"])
        for v, w, b in ((in32, "w_in", "b_in"), (x0, "w_pj", "b_pj")):
            want, mag = R.lin64(v, c["lin"][w], c["lin"][b])
            r = float((np.abs(R.emulate_mm(v, c["lin"][w], c["lin"][b], bf16).astype(np.float64) - want) / (TOL * mag + FLOOR)).max())
            worst = max(worst, r)
            assert r <= 0.5, (d_in, d_pj, biases, bf16, r)
    print(f"emulated error / bound, worst {worst:.3f}")


DEFECTS = ["row_off", "ge", "dec_first", "no_max", "drop_lo", "no_nan"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_are_caught(defect):
    """A faultless result (the reference itself; x and fx from the emulation) against a reference with one defect planted: the frame one row off, >= for >, the
    decrement before the zero test, no max_steps stop, the activations' lo plane dropped (planted into the emulated kernel), no NaN -> bos.  (a), (b) or (d)
    must fail on each -- and pass without one."""
    c = add_lin(make_case(17, "defects"), 1024, 512, False, True)
    B = c["B"]
    frame = c["frame"]
    good_state, good_lat = R.close(c["state"], c["latents"], frame, c["logit"], B, c["ldim"])
    in32, x0 = R.open_(c["state"], c["latents"], c["noise"], c["bos"], B)

    def opened(drop_lo):
        pad = lambda a: np.concatenate([a, filled(PAD, a.shape[1])])   # noqa: E731
        return dict(in32=pad(in32), x0=pad(x0), x=pad(R.emulate_mm(in32, c["lin"]["w_in"], c["lin"]["b_in"], False, drop_lo)),
                    fx=pad(R.emulate_mm(x0, c["lin"]["w_pj"], c["lin"]["b_pj"], False, drop_lo)))

    closed = dict(state=good_state, latents=good_lat)
    check_close("faultless", c, closed, good_state, good_lat)
    check_open("faultless", c, opened(False), c["state"], c["latents"], log=False)
    with pytest.raises(AssertionError):
        if defect == "drop_lo":
            check_open(defect, c, opened(True), c["state"], c["latents"], log=False)
        elif defect == "no_nan":
            w = R.open_(c["state"], c["latents"], c["noise"], c["bos"], B, defect)
            assert same_bits(in32, w[0]) and same_bits(x0, w[1])   # (d)'s exact comparison, against the defective reference
        else:
            bad_state, bad_lat = R.close(c["state"], c["latents"], frame, c["logit"], B, c["ldim"], defect)
            check_close(defect, c, closed, bad_state, bad_lat)


# ------------------------------------------------------------------------------------------------ GPU: (a) + (b), the books and the frame's place
@gpu
@pytest.mark.parametrize("B", LIST_B)
@pytest.mark.parametrize("op", ["finish", "fin", "fin_chain"])
def test_books_and_frame_place(pkg, op, B):
    """k_step_finish, k_skinny FIN and FIN + CHAIN on the crafted table: state and n_active integer for integer, the frame at row `step` bit-equal to what the
    launch produced (FINISH: the frame handed in; FIN: C), every other element of the latents, the inactive rows and the rows behind B as they were."""
    c = add_final(add_lin(make_case(B, "books", rot=1, noise=B % 2 == 1), 1024, 512, op == "fin_chain" and B % 3 == 0, True), 64, 1 if op == "fin_chain" and B % 3 == 0 else 0)
    got = run(pkg, op, c)
    name = f"{op} B{B}"
    assert got["launched"] == ({"k_step_finish": 1} if op == "finish" else {"k_skinny": 1}), (name, got["launched"])
    act = np.flatnonzero(c["state"]["active"][:B])
    if op == "finish":
        frame = c["frame"]
        assert untouched(got["in32"]) and untouched(got["x0"])
    elif op == "fin":
        frame = got["cur"]
        assert np.isfinite(frame[:B]).all() and same_bits(frame[B:], c["final"]["cur"][B:]) and untouched(got["in32"]) and untouched(got["x0"])
    else:   # chained: the frame is in the latents only, C (the Euler state) is not written: the next x0 goes to the other copy
        frame = np.array(c["frame"])
        for r in act:
            frame[r] = got["latents"][r, c["state"]["step"][r] * 32:(c["state"]["step"][r] + 1) * 32]
        assert np.isfinite(frame[act]).all() and same_bits(got["cur"], c["final"]["cur"]) and untouched(got["in32"])
    want_state, want_lat = R.close(c["state"], c["latents"], frame, c["logit"], B, c["ldim"])
    check_close(name, c, got, want_state, want_lat)


# ------------------------------------------------------------------------------------------------ GPU: (c) the frame's values
FRAME_CASES = [(op, K, w, LIST_B[(i + 3 * j + k) % len(LIST_B)]) for i, op in enumerate(("fin", "fin_chain")) for j, K in enumerate((64, 512)) for k, w in enumerate((0, 1, 2))]


def frame_check(pkg, name, c, got_frame, rows):
    """the rows `rows` of the frame against frame64 under the ln_mod + AXPY bound of test_gpu_step_linear, and bit for bit against the non-FIN instance of the same
    arithmetic (debug_step_linear: LN | MOD prologue, EPI_AXPY, the residual in place)."""
    f, B = c["final"], c["B"]
    weff = eff_weights(f)
    want, ab, absb = R.frame64(f["fx"][:B], f["shift"][:B], f["mscale"][:B], weff, f["bias"], f["cur"][:B], f["alpha"], f["eps"])
    bound = abs(f["alpha"]) * TOL * (ab + absb) + TOL * np.abs(f["cur"][:B].astype(np.float64)) + FLOOR
    check_bound(name, got_frame[rows], want[rows], bound[rows], TOL)
    sl = pkg.runtime.debug_step_linear(f["fx"][:B], f["W"], wfmt=f["wfmt"], bias=f["bias"], residual=f["cur"][:B], inplace=True, alpha=f["alpha"], epi=7, ln=True,
                                       eps=f["eps"], shift=f["shift"][:B], mscale=f["mscale"][:B])
    assert sl["k_skinny"] == 1 and same_bits(got_frame[rows], sl["out"][rows]), (name, "differs from the non-FIN instance", float(np.abs(got_frame[rows] - sl["out"][rows]).max()))
    return sl


@gpu
@pytest.mark.parametrize("op,K,wfmt,B", FRAME_CASES, ids=[f"k_skinny-{op}-K{K}-{WF[w]}-B{B}" for op, K, w, B in FRAME_CASES])
def test_frame_values(pkg, op, K, wfmt, B):
    c = add_final(add_lin(make_case(B, f"frame{K}{wfmt}"), 1024, 512, wfmt != 0, True), K, wfmt)
    got = run(pkg, op, c)
    assert got["launched"] == {"k_skinny": 1}
    if wfmt == 2:
        assert np.array_equal(got["w_eff"], eff_weights(c["final"])) and np.array_equal(got["w_scale"], SL.quantize_rows(c["final"]["W"])[2])
    act = np.flatnonzero(c["state"]["active"][:B])
    if op == "fin":
        frame, rows = got["cur"][:B], np.arange(B)
    else:
        frame, rows = np.zeros((B, 32), F32), act
        for r in act:
            frame[r] = got["latents"][r, c["state"]["step"][r] * 32:(c["state"]["step"][r] + 1) * 32]
    if rows.size:
        frame_check(pkg, f"k_skinny {op} K{K} {WF[wfmt]} B{B} frame", c, frame, rows)
    full = np.array(c["frame"])
    full[:B][rows] = frame[rows]
    check_close(f"{op} K{K} {WF[wfmt]} B{B}", c, got, *R.close(c["state"], c["latents"], full, c["logit"], B, 32))


@gpu
def test_frame_values_at_64_columns_with_bias(pkg):
    """FIN at N = ldim = 64, the edge of a.N <= 64: four column groups of the one block all store frames"""
    c = add_final(make_case(33, "n64", ldim=64), 512, 1, bias=True)
    got = run(pkg, "fin", c)
    assert got["launched"] == {"k_skinny": 1}
    frame_check(pkg, "k_skinny fin N64 K512 bf16 B33 frame", c, got["cur"][:33], np.arange(33))
    check_close("fin N64", c, got, *R.close(c["state"], c["latents"], got["cur"], c["logit"], 33, 64))


# ------------------------------------------------------------------------------------------------ GPU: (d) the opening's values
@gpu
@pytest.mark.parametrize("B", LIST_B)
def test_begin_without_linears(pkg, B):
    c = make_case(B, "begin", rot=10, noise=B % 2 == 0)
    got = run(pkg, "begin", c)
    assert got["launched"] == {"k_step_begin": 1} and got["x"] is None
    check_open(f"k_step_begin B{B}", c, got, c["state"], c["latents"])
    check_close(f"k_step_begin B{B} leaves the books", c, got, c["state"], c["latents"])


SCALAR = [(32, 24, 16, False, 5), (32, 24, 40, True, 17), (16, 16, 32, False, 33), (16, 1024, 512, True, 16), (64, 16, 16, True, 15), (64, 1024, 512, False, 256), (64, 300, 7, False, 1)]


@gpu
@pytest.mark.parametrize("ldim,d_in,d_pj,bf16,B", SCALAR, ids=[f"k_step_begin-ldim{l}-{i}x{p}-{'bf16' if b else 'f32'}-B{B}" for l, i, p, b, B in SCALAR])
def test_begin_scalar(pkg, ldim, d_in, d_pj, bf16, B):
    """the shapes step_open_mfma_ok refuses: d_in = 24 (no multiple of 16) at ldim 32, and ldim 16 / 64; several column blocks of 256 (1024 + 512)"""
    c = add_lin(make_case(B, "scalar", ldim=ldim, rot=9), d_in, d_pj, bf16, B % 2 == 1)
    got = run(pkg, "begin_lin", c)
    assert got["launched"] == {"k_step_begin": 1}, got["launched"]
    check_open(f"k_step_begin ldim{ldim} {d_in}x{d_pj} {'bf16' if bf16 else 'f32'} B{B}", c, got, c["state"], c["latents"])
    check_close("k_step_begin leaves the books", c, got, c["state"], c["latents"])


OPEN_CASES = list(_open_cases())
OPEN_IDS = [f"{i}x{p}-{'bias' if b else 'nobias'}-{'bf16' if h else 'f32'}-B{B}" for i, p, b, h, B in OPEN_CASES]


@gpu
@pytest.mark.parametrize("d_in,d_pj,biases,bf16,B", OPEN_CASES, ids=["k_step_begin_mm-" + s for s in OPEN_IDS])
def test_begin_mm(pkg, d_in, d_pj, biases, bf16, B):
    c = add_lin(make_case(B, "mm", rot=10, noise=d_in != 1024 or biases), d_in, d_pj, bf16, biases)
    got = run(pkg, "begin_lin", c)
    assert got["launched"] == {"k_step_begin_mm": 1}, got["launched"]
    check_open(f"k_step_begin_mm {d_in}x{d_pj} {'bias' if biases else 'nobias'} {'bf16' if bf16 else 'f32'} B{B}", c, got, c["state"], c["latents"])
    check_close("k_step_begin_mm leaves the books", c, got, c["state"], c["latents"])


@gpu
def test_begin_with_an_odd_stride_takes_the_scalar_kernel(pkg):
    """the matrix-core opening reads the latents and the noise in pairs: a row stride that is odd sends the launcher to k_step_begin, with the same results"""
    c = add_lin(make_case(17, "odd", rot=10), 16, 16, False, True)
    c["latents"] = np.concatenate([c["latents"], np.full((c["rows"], 1), np.nan, F32)], axis=1)
    got = pkg.runtime.debug_step_edge("begin_lin", c["state"], c["latents"], c["bos"], B=17, S=S, noise=c["noise"], lin=c["lin"])
    assert got["launched"] == {"k_step_begin": 1}
    check_open("k_step_begin odd lat_stride", c, got, c["state"], c["latents"])


@gpu
@pytest.mark.parametrize("d_in,d_pj,biases,bf16,B", OPEN_CASES, ids=["k_skinny-fin_chain-" + s for s in OPEN_IDS])
def test_chained_opening(pkg, d_in, d_pj, biases, bf16, B):
    """FIN + CHAIN at every width: the next step's x0 (rows active before the launch: open_() on the state and latents AFTER it; rows that were inactive: zeros),
    x = input_linear(frame, NaN -> bos) and fx = input_proj(x0).  One active row's frame holds a NaN element (from its residual).  The multi-pass widths run
    the tail's loop with reloaded weight fragments; (16, 16) its clamps."""
    c = make_case(B, "chain", rot=1, noise=d_in != 1024 or biases)
    act = np.flatnonzero(c["state"]["active"][:B])
    assert act.size
    c = add_final(add_lin(c, d_in, d_pj, bf16, biases), 64, (1 + (d_in // 16) % 2) if bf16 else 0, nan_row=int(act[-1]))
    got = run(pkg, "fin_chain", c)
    name = f"k_skinny fin_chain {d_in}x{d_pj} {'bias' if biases else 'nobias'} {'bf16' if bf16 else 'f32'} B{B}"
    assert got["launched"] == {"k_skinny": 1} and untouched(got["in32"]) and same_bits(got["cur"], c["final"]["cur"]), name
    r = int(act[-1])
    assert np.isnan(got["latents"][r, c["state"]["step"][r] * 32 + 5]), "the NaN element of the frame is stored as it is"
    frame = np.array(c["frame"])
    for a in act:
        frame[a] = got["latents"][a, c["state"]["step"][a] * 32:(c["state"]["step"][a] + 1) * 32]
    after, lat_after = R.close(c["state"], c["latents"], frame, c["logit"], B, 32)
    check_close(name, c, got, after, lat_after)
    check_open(name, c, got, after, got["latents"], in32=False, sel=act)
    idle = np.flatnonzero(c["state"]["active"][:B] == 0)
    if idle.size:   # rows that were inactive: x0 zeros, fx = input_proj(0) = the bias, x finite
        assert not got["x0"][idle].any() and np.isfinite(got["x"][idle]).all()
        want, mag = R.lin64(np.zeros((idle.size, 32), F32), c["lin"]["w_pj"], c["lin"]["b_pj"])
        check_bound(name + " fx of inactive rows", got["fx"][idle], want, TOL * mag + FLOOR, TOL)


# ------------------------------------------------------------------------------------------------ GPU: (e) one opening, whichever form
SEQ = [(17, 0, True), (33, 1, False), (5, 2, True), (256, 1, True), (16, 0, False)]


@gpu
@pytest.mark.parametrize("B,wfmt,noise", SEQ, ids=[f"B{B}-{WF[w]}-{'noise' if n else 'zeros'}" for B, w, n in SEQ])
def test_one_opening_whichever_form(pkg, B, wfmt, noise):
    """Four steps on the crafted table by three routes, each fed its own outputs (state, latents, cur = x0, the final layer's rows = fx (d_pj = K = 64), the EOS
    logit = x's first column), so that rows finish at different steps:
      A  FIN + CHAIN                      B  FIN, then BEGIN_LIN (k_step_begin_mm)                      C  FINISH on B's frame, then BEGIN_LIN.
    Contract: on every row that is active after a step the routes give x, fx, x0 bit for bit, and on EVERY row the same state and latents -- step_open.h's "a step
    opened either way starts from the same bits", on which graph replay == plain launches rests.  A row that is inactive after the step is not compared in x,
    fx, x0: the forms legitimately differ there (the chain leaves zeros in x0 for a row that was already inactive and multiplies the frame it computed but
    did not store; k_step_begin reads the noise row whenever step < max_steps and multiplies the last stored frame); its state and latents stay put and its
    x / fx are finite."""
    c = add_final(add_lin(make_case(B, "seq", rot=10, noise=noise), 48, 64, wfmt != 0, True), 64, wfmt)
    first = run(pkg, "begin_lin", c)
    assert first["launched"] == {"k_step_begin_mm": 1}
    thr = np.array(c["state"]["eos_threshold"])
    thr[np.isfinite(thr)] = 0.4 * c["rng"].standard_normal(int(np.isfinite(thr).sum()))   # x's first column is ~N(0, 1.1): EOS at different steps
    st0 = dict(c["state"], eos_threshold=thr.astype(F32))
    routes = {k: dict(state=st0, latents=c["latents"], cur=first["x0"], fx=first["fx"], logit=first["x"][:, 0].copy()) for k in "AB"}
    routes["A"]["logit"][:B] = routes["B"]["logit"][:B] = c["logit"][:B]   # the first step: the table's logits
    for step in range(4):
        a, b = routes["A"], routes["B"]
        fa = dict(c["final"], fx=a["fx"], cur=a["cur"])
        fb = dict(c["final"], fx=b["fx"], cur=b["cur"])
        ga = run(pkg, "fin_chain", c, state=a["state"], latents=a["latents"], logit=a["logit"], final=fa)
        gb = run(pkg, "fin", c, state=b["state"], latents=b["latents"], logit=b["logit"], final=fb)
        ob = run(pkg, "begin_lin", c, state=gb["state"], latents=gb["latents"])
        gc = run(pkg, "finish", c, state=b["state"], latents=b["latents"], logit=b["logit"], frame=gb["cur"])
        oc = run(pkg, "begin_lin", c, state=gc["state"], latents=gc["latents"])
        assert ga["launched"] == gb["launched"] == {"k_skinny": 1} and ob["launched"] == oc["launched"] == {"k_step_begin_mm": 1} and gc["launched"] == {"k_step_finish": 1}
        before = np.asarray(b["state"]["active"][:B])
        for k in R.STATE_I32:
            assert np.array_equal(ga["state"][k], gb["state"][k]) and np.array_equal(gc["state"][k], gb["state"][k]), (step, k)
        assert ga["state"]["n_active"] == gb["state"]["n_active"] == gc["state"]["n_active"] == int(gb["state"]["active"][:B].sum()), step
        assert same_bits(ga["latents"], gb["latents"]) and same_bits(gc["latents"], gb["latents"]), step
        idle = np.flatnonzero(before == 0)
        assert same_bits(gb["latents"][idle], b["latents"][idle]) and all(np.array_equal(gb["state"][k][idle], b["state"][k][idle]) for k in R.STATE_I32), step
        live = np.flatnonzero(gb["state"]["active"][:B])
        for what in ("x", "fx", "x0"):
            assert same_bits(ga[what][live], ob[what][live]), (step, what, "FIN + CHAIN against FIN, BEGIN_LIN", np.argwhere(bits(ga[what][live]) != bits(ob[what][live]))[:8].tolist())
            assert same_bits(oc[what][live], ob[what][live]), (step, what, "FINISH, BEGIN_LIN against FIN, BEGIN_LIN")
            assert np.isfinite(ga[what][:B]).all() and np.isfinite(ob[what][:B]).all(), (step, what)
        print(f"step {step}: {before.sum()} rows active before, {live.size} after")
        routes["A"] = dict(state=ga["state"], latents=ga["latents"], cur=ga["x0"], fx=ga["fx"], logit=ga["x"][:, 0].copy())
        routes["B"] = dict(state=gb["state"], latents=gb["latents"], cur=ob["x0"], fx=ob["fx"], logit=ob["x"][:, 0].copy())
    assert routes["B"]["state"]["n_active"] < st0["n_active"] or B == 1


# ------------------------------------------------------------------------------------------------ GPU: (f) refusals
@gpu
def test_refusals_before_any_launch(pkg):
    """every precondition of ptts_debug_step_edge answers PTTS_EINVAL and launches nothing -- neither in the hook's census nor in a caller's; a chained launch
    that skinny_fuse_supported or step_open_mfma_ok refuses is not launched in another form."""
    rt = pkg.runtime

    def base(**kw):
        return add_final(add_lin(make_case(5, "refuse", **kw), 16, 16, False, True), 64, 0)

    def st(c, **kw):
        s = R.copy_state(c["state"])
        for k, (r, v) in kw.items():
            s[k][r] = v
        return dict(c, state=s)

    c = base()
    wide = lambda a: np.concatenate([a, np.zeros((a.shape[0], 1), F32)], axis=1)   # noqa: E731
    c64 = add_final(add_lin(make_case(5, "refuse", ldim=64), 16, 16, False, True), 64, 0)
    bad = {
        "ldim % 4": ("begin", dict(c, bos=c["bos"][:30])),
        "ldim 68": ("begin", dict(c, bos=np.zeros(68, F32), latents=np.zeros((7, S * 68), F32))),
        "B = 0": ("begin", dict(c, B=0)),
        "B above the rows held": ("begin", dict(c, B=8)),
        "B = 257": ("begin", dict(make_case(257, "refuse"))),
        "step < 0": ("finish", st(c, step=(1, -1))),
        "step > max_steps": ("begin", st(c, step=(0, 5), max_steps=(0, 4))),
        "max_steps > S": ("begin", st(c, max_steps=(2, S + 1))),
        "active at step == max_steps": ("fin", st(c, step=(3, 4), max_steps=(3, 4), active=(3, 1))),
        "FIN: K = 520": ("fin", add_final(base(), 520, 0)),
        "FIN: ldmod % 4": ("fin", dict(c, final=dict(c["final"], shift=c["final"]["shift"][:, :66], mscale=c["final"]["mscale"][:, :66]))),
        "FIN: N != ldim": ("fin", dict(c, final=dict(c["final"], W=c["final"]["W"][:16], bias=c["final"]["bias"][:16], cur=c["final"]["cur"][:, :16]))),
        "CHAIN: d_in = 24": ("fin_chain", add_final(add_lin(make_case(5, "refuse"), 24, 16, False, True), 64, 0)),
        "CHAIN: N = 64": ("fin_chain", c64),
        "CHAIN: epi != AXPY": ("fin_chain", dict(c, final=dict(c["final"], epi=4))),
        "CHAIN: f32 linears under bf16 step weights": ("fin_chain", dict(c, final=dict(c["final"], wfmt=1))),
        "CHAIN: bf16 linears under f32 step weights": ("fin_chain", add_final(add_lin(make_case(5, "refuse"), 16, 16, True, True), 64, 0)),
        "CHAIN: odd lat_stride": ("fin_chain", dict(c, latents=wide(c["latents"]), S=S)),
        "CHAIN: odd chain_noise_stride": ("fin_chain", dict(c, noise=wide(c["noise"]))),
    }
    rt.launch_counts(True)
    try:
        for what, (op, a) in bad.items():
            with pytest.raises(pkg.PttsError) as e:
                rt.debug_step_edge(op, a["state"], a["latents"], a["bos"], B=a["B"], S=a.get("S"), noise=a["noise"], eos_logit=a["logit"], frame=a["frame"] if op == "finish" else None,
                                   lin=a["lin"] if op in ("begin_lin", "fin_chain") else None, final=a["final"] if op in ("fin", "fin_chain") else None)
            assert e.value.code == rt.PTTS_EINVAL, what
            assert rt.launch_counts(True) == {}, what
        for null in ("bos", "step", "n_active", "eos_logit", "cur", "w_in", "x"):
            with pytest.raises(pkg.PttsError) as e:
                rt.debug_step_edge("fin_chain", c["state"], c["latents"], c["bos"], B=5, noise=c["noise"], eos_logit=c["logit"], lin=c["lin"], final=c["final"], null=(null,))
            assert e.value.code == rt.PTTS_EINVAL and rt.launch_counts(True) == {}, null
        # ... and their neighbour is taken, and counted in the caller's census too
        assert run(pkg, "fin_chain", c)["launched"] == {"k_skinny": 1} and rt.launch_counts(True) == {"k_skinny": 1}
        assert run(pkg, "finish", c)["launched"] == {"k_step_finish": 1} and run(pkg, "begin", c)["launched"] == {"k_step_begin": 1}
        assert rt.launch_counts(True) == {"k_step_finish": 1, "k_step_begin": 1}
    finally:
        rt.launch_counts(False)
