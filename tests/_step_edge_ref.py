"""The opening and the closing of an AR step in plain numpy (f64 where values are computed, integers where the books are kept): the reference side of
tests/test_gpu_step_edge.py.  No GPU, no kernel code restated: finish() follows the Go loop, open_() the construction of the step's input, lin64 / frame64
the two products.  emulate_mm alone restates a kernel's arithmetic (step_open.h so_tile), to show that the bound has room for it.

The state is a dict {name: int32 [rows]} over STATE_I32 plus "eos_threshold" (f32 [rows]) and "n_active" (int) -- kernels.h StepState.  countdown -1 is the
reference's nil *int.  Every function leaves its arguments unchanged and touches rows [0, B) only.

`defect` plants one wrong reading of the rules into the reference (test_planted_defects_are_caught): the checks must tell it from the right one."""
import numpy as np

from _kernel_ref import split

F32 = np.float32
STATE_I32 = ("kv_len", "active", "step", "countdown", "n_frames", "eos_step", "max_steps", "frames_after_eos", "broke")


def copy_state(s):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.items()}


# ------------------------------------------------------------------------------------------------ the books
def finish(state, logit, B, defect=None):
    """One pass of the generation loop's tail per active row (runtime_native_safetensors.go:176-192) and the loop's own bound (`for step := range maxSteps`,
    :155): the frame is appended (n_frames), an EOS (flow_lm.go:281: logit > threshold, strictly -- a NaN logit is none) arms the countdown once with
    frames_after_eos and is remembered in eos_step, an armed countdown at 0 breaks (broke) and is decremented otherwise; a row whose next step would be
    max_steps has run out.  A row that leaves takes one off n_active."""
    s = copy_state(state)
    for r in range(B):
        if not s["active"][r]:
            continue
        st = int(s["step"][r])
        s["n_frames"][r] = st + 1                                           # :176 latentFrames = append(latentFrames, frame)
        lg, thr = F32(logit[r]), F32(s["eos_threshold"][r])
        is_eos = bool(lg >= thr) if defect == "ge" else bool(lg > thr)      # flow_lm.go:281
        cd = int(s["countdown"][r])
        done = False
        if is_eos and cd < 0:                                               # :178 isEOS && eosCountdown == nil
            cd = int(s["frames_after_eos"][r])
            s["eos_step"][r] = st
        if cd >= 0:                                                         # :184 eosCountdown != nil
            if defect == "dec_first":
                cd -= 1
                if cd == 0:
                    done = True
                    s["broke"][r] = 1
            elif cd == 0:                                                   # :185-186 break
                done = True
                s["broke"][r] = 1
            else:
                cd -= 1                                                     # :189
        s["countdown"][r] = cd
        s["step"][r] = st + 1
        s["kv_len"][r] += 1                                                 # one more key in the cache
        if defect != "no_max" and st + 1 >= int(s["max_steps"][r]):         # :155 for step := range maxSteps
            done = True
        if done:
            s["active"][r] = 0
            s["n_active"] = int(s["n_active"]) - 1
    return s


def go_loop_frames(logits, thr, fae, max_steps):
    """The Go loop for ONE utterance, written down as it stands (:155-201) -> (frames collected, 1 if it left through the break, the step at which the
    countdown was armed or -1)."""
    frames, broke, eos_step = 0, 0, -1
    countdown = None
    for step in range(max_steps):
        frames += 1                                   # :176 append
        is_eos = bool(F32(logits[step]) > F32(thr))
        if is_eos and countdown is None:              # :178
            countdown = fae
            eos_step = step
        if countdown is not None:                     # :184
            if countdown == 0:
                broke = 1
                break
            countdown -= 1
    return frames, broke, eos_step


def close(state, latents, frame, logit, B, ldim, defect=None):
    """The step's end: the frame of an active row goes to row `step` of its latents (the value before the step), then the books.  -> (state, latents)"""
    lat = np.array(latents, F32)
    S = lat.shape[1] // ldim
    for r in range(B):
        if state["active"][r]:
            at = int(state["step"][r])
            if defect == "row_off":
                at = (at + 1) % S
            lat[r, at * ldim:(at + 1) * ldim] = frame[r]
    return finish(state, logit, B, defect), lat


# ------------------------------------------------------------------------------------------------ the opening
def open_(state, latents, noise, bos, B, defect=None):
    """The step's input: the previous frame with every NaN element replaced by bos's (step 0: the BOS marker is all NaN, so bos itself;
    runtime_native_safetensors.go:246-253, tensor_util.go:259-268), and the flow's starting point: the noise row of this step, or zeros -- without a noise
    buffer, and for a row that has no step left (step == max_steps).  -> (in32 [B, ldim], x0 [B, ldim])"""
    ldim = bos.shape[0]
    in32, x0 = np.zeros((B, ldim), F32), np.zeros((B, ldim), F32)
    for r in range(B):
        st = int(state["step"][r])
        if st == 0:
            in32[r] = bos
        else:
            v = np.array(latents[r, (st - 1) * ldim:st * ldim], F32)
            in32[r] = v if defect == "no_nan" else np.where(np.isnan(v), bos, v)
        if noise is not None and st < int(state["max_steps"][r]):
            x0[r] = noise[r, st * ldim:(st + 1) * ldim]
    return in32, x0


def as_f32(w):
    """weights as the kernels read them: bf16 bits (uint16) are the f32 values of those bits"""
    w = np.asarray(w)
    return (w.astype(np.uint32) << 16).view(F32) if w.dtype == np.uint16 else np.asarray(w, F32)


def lin64(v, W, b):
    """v W^T + b in f64 with the bound's |.| sum: -> (out [B, N], sum_k |w v| + |b|)"""
    v64, w64 = np.asarray(v, np.float64), as_f32(W).astype(np.float64)
    b64 = np.zeros(w64.shape[0]) if b is None else np.asarray(b, np.float64)
    return v64 @ w64.T + b64, np.abs(v64) @ np.abs(w64).T + np.abs(b64)


def emulate_mm(v, W, b, w_bf16, drop_lo=False):
    """step_open.h so_tile in numpy f32: the activations as bf16 hi + lo planes, bf16 weights as they are (two 32-deep matrix steps: W hi, W lo of the
    activations), f32 weights split the same way with the lo * lo product dropped (three steps: wh xh, wh xl, wl xh); one f32 accumulator, the bias last."""
    v = np.ascontiguousarray(v, F32)
    assert v.shape[1] == 32
    xh, xl = split(v)
    w = as_f32(W)
    if w_bf16:
        acc = xh @ w.T
        if not drop_lo:
            acc = acc + xl @ w.T
    else:
        wh, wl = split(w)
        acc = xh @ wh.T
        if not drop_lo:
            acc = acc + xl @ wh.T
        acc = acc + xh @ wl.T
    return acc + (F32(0.0) if b is None else np.asarray(b, F32))


# ------------------------------------------------------------------------------------------------ the frame
def frame64(fx, shift, mscale, W, bias, R, alpha, eps):
    """flowFinalLayer.Forward (flow_net.go:205-239) and the Euler update: LayerNorm without affine (biased variance, linear.go:295-309), * (1 + scale) + shift,
    the product plus bias, R + alpha * (...), all f64.  -> (frame [B, N], sum_k |y w| [B, N], |bias| [N])"""
    K = W.shape[1]
    x = np.asarray(fx, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    y = (x - mean) / np.sqrt(((x - mean) ** 2).mean(axis=1, keepdims=True) + eps)
    y = y * (1.0 + np.asarray(mscale, np.float64)[:, :K]) + np.asarray(shift, np.float64)[:, :K]
    w64 = np.asarray(W, np.float64)
    b64 = np.zeros(w64.shape[0]) if bias is None else np.asarray(bias, np.float64)
    return np.asarray(R, np.float64) + alpha * (y @ w64.T + b64), np.abs(y) @ np.abs(w64).T, np.abs(b64)
