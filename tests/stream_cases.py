"""The session's stream contract under a stalled stream (include/dinov2_hip.h "stream contract", DESIGN.md "Stream contract").

Every scenario is one chain of library calls, written once and run twice on fresh sessions of the tiny fixtures:
  calm     the session is synchronised after every step;
  stalled  every output buffer is filled with NaN and the device synchronised BEFORE the chain starts; api.stream_delay (a bounded wait
           of STALL_MS on the session's stream) is queued in front of every step; nothing synchronises between the steps but the library
           itself; one synchronisation at the end.
The criterion is check_exact, bit equality of every output of every step between the two runs: the forward is bit-reproducible, so no
tolerance is involved.  Host results are copied the moment their call returns -- before anything else could complete them -- so "complete on
return" is held by the same comparison.

STEPS declares every step as ASYNC ("asynchronous in steady state": the shape, the query list and the scratch sizes have been seen before --
the steps named warm / *1 see them first) or WAITS, with the wait of WAIT_SITES the step runs into:
  ASYNC  the stream is queried right after the call returns and must still be busy: the step really ran behind the stall, and the
         header's word "asynchronous" is held to the code;
  WAITS  host outputs hold their final values on return (the copy taken on return equals the calm run's; where the test owns the buffer it
         starts as NaN).

STALL_MS.  The stall must outlast the host time a call needs to enqueue its work.  Measured with a host clock around the call, on an MI355X,
with the forward code of the parent commit (this work changes nothing a forward enqueues): the longest asynchronous chain step on the tiny
models is scenario G's steady-state predict_list_device of four images, MEASURED_ENQUEUE_MS = 0.124 ms as the worst of 50 calls (median
0.114 ms); scenario A's chain step (a device copy, a predict_device of 2 images at 70 x 98, two device copies) took 0.102 ms at worst, a
steady-state predict_attention_device 0.081 ms.  A loaded host can stall the launch thread, hence a margin of at least 4: STALL_MS >=
4 * MEASURED_ENQUEUE_MS = 0.5 ms, and never above the op's cap of 100 ms.  STALL_MS = 20 is 160 times the measured time: the margin costs
little (the longest chain, F, stalls for a third of a second in all) and the ASYNC assertion, which is the proof that the stall was long
enough, then survives a launch thread that is held up for milliseconds.  No scenario accumulates more than a second of stall."""
import ctypes as C
import os

import numpy as np

ASYNC, WAITS = "async", "waits"
MEASURED_ENQUEUE_MS = 0.124  # worst host time of the longest asynchronous chain step (docstring; DESIGN.md "Stream contract")
STALL_MS = 20
H, R, NCLS, PS, HEADS, LAYERS = 128, 4, 10, 14, 2, 2  # the tiny fixtures (synth.CONFIGS["tiny"], 4 registers, 10 classes)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dinov2.cpp_amd", "csrc")

# The waits of the session code a step can run into: name -> (file under csrc/, line, what it keeps safe).  tests/test_stream_cases.py
# checks that each line holds a wait and that DESIGN.md's table has a row for it.
WAIT_SITES = {
    "reserve":        ("model.cpp", 78, "a scratch buffer is freed and reallocated: work in flight may still use the old one"),
    "apply_carve":    ("model.cpp", 141, "the workspace grows: captured graphs and work in flight point into the old one"),
    "prepare_pos":    ("model.cpp", 261, "pos_stage (host) is rewritten by the next shape; the call returns after the copy has landed"),
    "list_pos":       ("model.cpp", 479, "list_pos_stage (host) is rewritten by the next list with a new grid"),
    "list_items":     ("model.cpp", 498, "list_items_host is rewritten by the next list with another work table"),
    "fetch_outputs":  ("model.cpp", 617, "host outputs of predict / fetch are complete on return"),
    "list_outputs":   ("model.cpp", 617, "host outputs of predict_list are complete on return (the same copy-out, one run per image size)"),
    "attn_queries":   ("extras.cpp", 107, "the device query list is replaced: an attention kernel in flight may still read the old one"),
    "tapped_outputs": ("extras.cpp", 138, "host taps / attention rows (staged in session scratch) are complete on return"),
    "dense_outputs":  ("extras.cpp", 271, "host label / value / logit maps are complete on return"),
    "match":          ("resident.cpp", 83, "host results of match_tokens are complete on return"),
    "bank_add":       ("resident.cpp", 240, "a returned bank is complete; host rows were read"),
    "bank_topk":      ("resident.cpp", 290, "host results of bank_topk are complete on return"),
    "kmeans":         ("resident.cpp", 396, "host results of kmeans_tokens are complete on return"),
    "pca3":           ("pca.cpp", 185, "host results of pca3 are complete on return"),
    "pageable_h2d":   (None, 0, "no wait of the library's: the runtime may hold the caller until a copy from pageable memory has been staged; "
                                "the header promises asynchrony for page-locked input only"),
}

# scenario -> step -> (ASYNC | WAITS, wait site or None).  A step of a chain that is not declared here is a KeyError.
STEPS = {
    "A": {"warm": (WAITS, "prepare_pos"), "chain": (ASYNC, None)},
    "B": {"warm": (WAITS, "prepare_pos"), **{"p%d" % i: (ASYNC, None) for i in range(6)}},
    "C": {"large1": (WAITS, "prepare_pos"), "small": (WAITS, "prepare_pos"), "large2": (WAITS, "prepare_pos"), "again": (ASYNC, None)},
    "D": {"small": (WAITS, "prepare_pos"), "larger": (WAITS, "apply_carve"), "again": (ASYNC, None)},
    "E": {"warm": (WAITS, "prepare_pos"), "layers1": (ASYNC, None), "layers2": (ASYNC, None), "attn1": (WAITS, "attn_queries"),
          "attn2": (ASYNC, None), "attn3": (WAITS, "attn_queries"), "attn4": (ASYNC, None)},
    "F": {"predict": (WAITS, "fetch_outputs"), "layers": (WAITS, "fetch_outputs"), "attention": (WAITS, "fetch_outputs"),
          "layers_alone": (WAITS, "tapped_outputs"), "dense": (WAITS, "dense_outputs"),
          "dev_fetch": (ASYNC, None), "fetch": (WAITS, "fetch_outputs"), "dev_match": (ASYNC, None), "match": (WAITS, "match"),
          "dev_add": (ASYNC, None), "bank_add": (WAITS, "bank_add"), "dev_topk": (ASYNC, None), "bank_topk": (WAITS, "bank_topk"),
          "dev_kmeans": (ASYNC, None), "kmeans": (WAITS, "kmeans"), "dev_pca": (ASYNC, None), "pca3": (WAITS, "pca3")},
    "G": {"list1": (WAITS, "list_items"), "list2": (WAITS, "list_items"), "list2_again": (ASYNC, None), "host_list": (WAITS, "list_outputs")},
    "H": {"warm_stalled": (WAITS, "prepare_pos"), "warm_free": (WAITS, "prepare_pos"), "stalled": (ASYNC, None),
          "free": (WAITS, "fetch_outputs")},
    "K": {"warm": (WAITS, "prepare_pos"), "warm_other": (WAITS, "fetch_outputs"), "forward": (ASYNC, None), "bank_add": (WAITS, "bank_add"),
          "topk_other": (WAITS, "bank_topk")},
    "I": {"warm": (WAITS, "prepare_pos"), "pinned_dev": (ASYNC, None), "pageable_dev": (WAITS, "pageable_h2d"),
          "pinned_null": (ASYNC, None), "fetch_pinned": (WAITS, "fetch_outputs"), "pageable_null": (WAITS, "pageable_h2d"),
          "fetch_pageable": (WAITS, "fetch_outputs")},
}


def images(B, h, w, seed):
    return np.random.default_rng(seed).standard_normal((B, 3, h, w)).astype(np.float32)


def patches(h, w):
    return (h // PS) * (w // PS)


def check_exact(got, exp, what):
    """(ok, message): the same shape, type and bytes (-0 is not +0; a NaN equals only the same NaN)."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return False, f"{what}: {got.dtype}{got.shape} against {exp.dtype}{exp.shape}"
    bad = got.reshape(-1).view(np.uint8) != exp.reshape(-1).view(np.uint8)
    if not bad.any():
        return True, ""
    i = int(np.flatnonzero(bad)[0]) // got.dtype.itemsize
    return False, f"{what}: {int(bad.sum())} bytes of {got.size} elements differ, first element {i}: {got.reshape(-1)[i]!r} against {exp.reshape(-1)[i]!r}"


class _Dry:
    """Stands in for a device array / handle when a chain is only walked for its step names (no device)."""
    ptr, _h = 0, None

    def __init__(self, shape=()):
        self.shape, self.nbytes = tuple(shape), 0

    def __iter__(self):  # (arrays, struct) pairs unpack
        return iter((_Dry(), _Dry()))


class Run:
    """One pass of a chain.  dry: no device; step() only records the names."""

    def __init__(self, api, sid, stalled, sess=None, stream=None, model=None, dry=False):
        self.api, self.sid, self.stalled, self.sess, self.stream, self.model, self.dry = api, sid, stalled, sess, stream, model, dry
        self.started = False
        self.outputs, self.inputs, self.objects, self.host, self.busy, self.order, self.keep = {}, {}, {}, {}, {}, [], []

    # -- what a chain allocates, all of it before its first step (a device allocation synchronises; a repeat of the chain gets the same buffers)
    def dev(self, name, shape):
        if name not in self.outputs:
            assert not self.started, "output buffers are allocated and filled with NaN before the chain starts"
            self.outputs[name] = _Dry(shape) if self.dry else self.api.DeviceArray(shape, fill_nan=True)
        return self.outputs[name]

    def upload(self, name, host):
        if name not in self.inputs:
            assert not self.started
            self.inputs[name] = _Dry(host.shape) if self.dry else self.api.DeviceArray.from_host(host)
        return self.inputs[name]

    def make(self, name, fn):
        if name not in self.objects:
            assert not self.started
            self.objects[name] = _Dry() if self.dry else fn()
        return self.objects[name]

    def step(self, name, fn, sess=None, stream=None):
        kind, _ = STEPS[self.sid][name]
        self.order.append(name)
        self.started = True
        if self.dry:
            return
        sess, stream = sess or self.sess, stream or self.stream
        if self.stalled:
            self.api.stream_delay(stream, STALL_MS)
        res = fn()
        if self.stalled and kind == ASYNC:
            self.busy.setdefault(name, []).append(not stream.query())
        self.keep.append(res)  # (the caller's buffers outlive the chain, as the contract asks of them)
        for k, v in (res or {}).items():
            self.host[name + "." + k] = np.array(v, copy=True)  # as it stands on return
        if not self.stalled:
            sess.sync()

    def finish(self, sessions=()):
        """The one synchronisation at the end -- dinov2_hip_session_sync, which is what the header tells a caller to use before reading device
        outputs -- and then every device buffer to the host."""
        for s in sessions or (self.sess,):
            s.sync()
        out = dict(self.host)
        out.update({"dev." + k: a.to_host() for k, a in self.outputs.items()})
        return out

    def free(self):
        for a in list(self.outputs.values()) + list(self.inputs.values()):
            a.free()
        for o in self.objects.values():
            if hasattr(o, "close"):
                o.close()


# --------------------------------------------------------------------------------------------------------------- raw C-ABI calls
def _nan_host(api, shape, pinned):
    a = api.pinned_empty(shape) if pinned else np.empty(shape, np.float32)
    a.fill(np.nan)
    return a


def stale_host(api, shape, dtype=np.float32):
    """A page-locked host array of 0xff bytes (NaN; -1; 255).  Page-locked on purpose: the runtime finishes a copy into PAGEABLE memory before
    hipMemcpyAsync returns, so only a page-locked result shows whether the library waited for it ("Stream contract")."""
    a = api.pinned_empty(shape, dtype)
    a.view(np.uint8).fill(0xff)
    return a


def host_outputs(api, B, h, w, classify, pinned=True):
    """(dict of NaN-filled host arrays, the Output naming them) of a classify / feature predict of B images."""
    out = {"cls": _nan_host(api, (B, H), pinned), "patch_tokens": _nan_host(api, (B, patches(h, w) + (R if classify else 0), H), pinned)}
    if classify:
        out["logits"], out["probs"] = _nan_host(api, (B, NCLS), pinned), _nan_host(api, (B, NCLS), pinned)
    o = api.Output()
    for k, v in out.items():
        setattr(o, k, C.c_void_p(v.ctypes.data))
    return out, o


def predict_raw(api, sess, data_ptr, B, h, w, classify, out, in_on_device):
    """dinov2_hip_predict with any combination of host / device input and host / device / no outputs (`out`: an Output or None)."""
    i = api.Input(data_ptr, B, h, w, api.RGB_CHW, int(in_on_device))
    api._call(api.lib().dinov2_hip_predict, sess._h, C.byref(i), C.byref(out) if out is not None else None, api.CLASSIFY if classify else 0)


def fetch_raw(api, sess, out):
    api._call(api.lib().dinov2_hip_fetch, sess._h, C.byref(out))


def device_outputs(c, tag, B, h, w, classify):
    """The four device output buffers of one predict_device, as keyword arguments."""
    kw = {"cls_ptr": c.dev(tag + ".cls", (B, H)).ptr, "patch_ptr": c.dev(tag + ".patch", (B, patches(h, w) + (R if classify else 0), H)).ptr}
    if classify:
        kw.update(logits_ptr=c.dev(tag + ".logits", (B, NCLS)).ptr, probs_ptr=c.dev(tag + ".probs", (B, NCLS)).ptr)
    return kw


# --------------------------------------------------------------------------------------------------------------- the chains
def chain_A(c, classify=True):
    """Caller's stream: stall, device copy of the images into a buffer full of NaN, predict_device from that buffer, device copies of the
    logits and tokens into second buffers -- all on S.  A session that is not ordered behind the producer reads NaN; a consumer that is not
    ordered behind the session copies NaN."""
    B, h, w = 2, 70, 98
    src = c.upload("x", images(B, h, w, 1))
    stage = c.dev("stage", (B, 3, h, w))
    wkw, kw = device_outputs(c, "warm", B, h, w, classify), device_outputs(c, "out", B, h, w, classify)
    first = "logits" if classify else "cls"
    lo, tok = c.outputs["out." + first], c.outputs["out.patch"]
    lo2, tok2 = c.dev("copy." + first, lo.shape), c.dev("copy.patch", tok.shape)
    c.step("warm", lambda: c.sess.predict_device(src.ptr, B, h, w, classify=classify, **wkw))

    def chain():
        c.stream.copy(stage, src)
        c.sess.predict_device(stage.ptr, B, h, w, classify=classify, **kw)
        c.stream.copy(lo2, lo)
        c.stream.copy(tok2, tok)
    c.step("chain", chain)


def chain_B(c, classify=True):
    """Six steady-state predict_device calls alternating between two inputs, into six distinct output sets."""
    B, h, w = 2, 56, 84
    x = [c.upload("x%d" % k, images(B, h, w, 10 + k)) for k in range(2)]
    kws = [device_outputs(c, "p%d" % i, B, h, w, classify) for i in range(6)]
    wkw = device_outputs(c, "warm", B, h, w, classify)
    c.step("warm", lambda: c.sess.predict_device(x[1].ptr, B, h, w, classify=classify, **wkw))
    for i in range(6):
        c.step("p%d" % i, lambda i=i: c.sess.predict_device(x[i % 2].ptr, B, h, w, classify=classify, **kws[i]))


def chain_C(c, classify=True):
    """Shape changes inside the workspace's capacity: large, small, large -- the re-carve (with ln_fold: its statistics memset) and the
    position-embedding restage against a forward in flight -- and the large shape once more in steady state."""
    big, small = (3, 70, 98), (1, 28, 42)
    xb, xs = c.upload("xb", images(*big, 20)), c.upload("xs", images(*small, 21))
    plan = [("large1", xb, big), ("small", xs, small), ("large2", xb, big), ("again", xb, big)]
    kws = [device_outputs(c, name, *shape, classify) for name, _, shape in plan]
    for (name, x, shape), kw in zip(plan, kws):
        c.step(name, lambda x=x, shape=shape, kw=kw: c.sess.predict_device(x.ptr, *shape, classify=classify, **kw))


def chain_D(c, classify=True):
    """Workspace growth mid-chain: small, then larger (a reallocation); the earlier device outputs stay intact."""
    small, big = (1, 28, 42), (3, 70, 98)
    xs, xb = c.upload("xs", images(*small, 30)), c.upload("xb", images(*big, 31))
    plan = [("small", xs, small), ("larger", xb, big), ("again", xb, big)]
    kws = [device_outputs(c, name, *shape, classify) for name, _, shape in plan]
    for (name, x, shape), kw in zip(plan, kws):
        c.step(name, lambda x=x, shape=shape, kw=kw: c.sess.predict_device(x.ptr, *shape, classify=classify, **kw))


def chain_E(c, classify=True):
    """predict_layers_device and predict_attention_device twice each, with different layer / query lists and all keys or patch keys: each
    call's rows belong to its own list.  The two query lists have one length, so the list's device buffer is replaced in place."""
    B, h, w = 2, 56, 84
    P, T = patches(h, w), 1 + R + patches(h, w)
    x = c.upload("x", images(B, h, w, 40))
    wkw = device_outputs(c, "warm", B, h, w, classify)
    l1, l2 = c.dev("layers1", (2, B, P, H)), c.dev("layers2", (1, B, P, H))
    q1, q2 = [0, 3, 7], [1, 5, T - 1]
    a = [c.dev("attn1", (1, B, HEADS, 3, T)), c.dev("attn2", (2, B, HEADS, 3, P)), c.dev("attn3", (2, B, HEADS, 3, P)),
         c.dev("attn4", (1, B, HEADS, 3, T))]
    c.step("warm", lambda: c.sess.predict_device(x.ptr, B, h, w, classify=classify, **wkw))
    c.step("layers1", lambda: c.sess.predict_layers_device(x.ptr, B, h, w, [1, 2], classify=classify, layer_patch_ptr=l1.ptr))
    c.step("layers2", lambda: c.sess.predict_layers_device(x.ptr, B, h, w, [0], norm=False, classify=classify, layer_patch_ptr=l2.ptr))
    c.step("attn1", lambda: c.sess.predict_attention_device(x.ptr, B, h, w, [2], a[0], q1, "all", classify=classify))
    c.step("attn2", lambda: c.sess.predict_attention_device(x.ptr, B, h, w, [1, 2], a[1], q1, "patches", classify=classify))
    c.step("attn3", lambda: c.sess.predict_attention_device(x.ptr, B, h, w, [1, 2], a[2], q2, "patches", classify=classify))
    c.step("attn4", lambda: c.sess.predict_attention_device(x.ptr, B, h, w, [1], a[3], q2, "all", classify=classify))


def chain_F(c, classify=True):
    """Host-output calls queued behind a stall, and the calls that read resident tokens directly after an unsynchronised predict_device
    (whose input alternates, so that tokens of the forward before it would be noticed)."""
    api, s = c.api, c.sess
    B, h, w = 2, 56, 84
    P = patches(h, w)
    xh = [images(B, h, w, 50), images(B, h, w, 51)]
    xd = [c.upload("x%d" % k, xh[k]) for k in range(2)]
    rng = np.random.default_rng(52)
    head = c.make("head", lambda: api.DenseHead(c.model, [1, 2], rng.standard_normal((5, 2 * H)).astype(np.float32) * 0.05,
                                                rng.standard_normal(5).astype(np.float32)))
    bank = c.make("bank", lambda: api.Bank(c.model, H, 4 * P))
    pred, po = c.make("predict_out", lambda: host_outputs(api, B, h, w, classify))
    fet, fo = c.make("fetch_out", lambda: host_outputs(api, B, h, w, classify))

    def predict():
        predict_raw(api, s, xh[0].ctypes.data, B, h, w, classify, po, 0)
        return pred

    def layers():
        r = s.predict_layers(xh[1], [1, 2], return_class_token=True, classify=classify)
        c.keep.append(r)
        return {"patch%d" % k: d["patch_tokens"] for k, d in enumerate(r["layers"])} | {"cls%d" % k: d["cls"] for k, d in enumerate(r["layers"])} | \
               {"logits": r["logits"]}

    def attention():
        rows, r = s.predict_attention(xh[0], [1, 2], [0, 2, 9], "patches", classify=classify, return_outputs=True)
        return {"rows": rows, **r}

    taps = c.make("taps_alone", lambda: _nan_host(api, (2, B, P, H), True))

    def layers_alone():  # out == NULL: the staged taps are the call's only host output, and predict_tapped's own wait the only one
        ids = (C.c_int32 * 2)(1, 2)
        ly = api.Layers(ids, 2, 1, api.LAYERS_TOKENS, taps.ctypes.data, None, None, 0)
        i = api.Input(xh[0].ctypes.data, B, h, w, api.RGB_CHW, 0)
        api._call(api.lib().dinov2_hip_predict_layers, s._h, C.byref(i), None, C.byref(ly), api.CLASSIFY if classify else 0)
        return {"patch": taps}

    oh, ow = 40, 61
    dense_out = c.make("dense_out", lambda: {"labels": stale_host(api, (B, oh, ow), np.uint8), "value": stale_host(api, (B, oh, ow)),
                                             "logits": stale_host(api, (B, P, 5))})
    match_out = c.make("match_out", lambda: {"idx_ab": stale_host(api, (P,), np.int32), "sim_ab": stale_host(api, (P,)),
                                             "idx_ba": stale_host(api, (P,), np.int32), "sim_ba": stale_host(api, (P,))})
    topk_out = c.make("topk_out", lambda: {"idx": stale_host(api, (B, 3), np.int32), "sim": stale_host(api, (B, 3))})
    km_out = c.make("kmeans_out", lambda: {"labels": stale_host(api, (P,), np.int32), "sim": stale_host(api, (P,)),
                                           "centers": stale_host(api, (3, H)), "counts": stale_host(api, (3,), np.int32)})
    km_init = np.array([0, 7, 15], np.int32)
    flags = api.CLASSIFY if classify else 0

    def dense():
        do = api.DenseOut(oh, ow, dense_out["labels"].ctypes.data, dense_out["value"].ctypes.data, dense_out["logits"].ctypes.data, 0)
        i = api.Input(xh[1].ctypes.data, B, h, w, api.RGB_CHW, 0)
        api._call(api.lib().dinov2_hip_predict_dense, s._h, C.byref(i), None, head._h, C.byref(do), flags)
        return dense_out

    def fetch():
        fetch_raw(api, s, fo)
        return fet

    def match():
        m = api.Match(None, None, P, P, H, 0, 1, 0, *(match_out[k].ctypes.data for k in ("idx_ab", "sim_ab", "idx_ba", "sim_ba")))
        api._call(api.lib().dinov2_hip_match_tokens, s._h, C.byref(m))
        return match_out

    def bank_topk():
        t = api.TopK(api.Rows(api.ROWS_LAST_CLS, None, B, H, 0, 0), 3, topk_out["idx"].ctypes.data, topk_out["sim"].ctypes.data)
        api._call(api.lib().dinov2_hip_bank_topk, s._h, bank._h, C.byref(t))
        return topk_out

    def kmeans():
        it, conv = C.c_int32(-1), C.c_int32(-1)
        km = api.KMeans(api.Rows(api.ROWS_LAST_PATCHES, None, P, H, 1, 0), 0, 3, 3, api.KMEANS_INIT_ROWS, None, km_init.ctypes.data,
                        km_out["labels"].ctypes.data, km_out["sim"].ctypes.data, km_out["centers"].ctypes.data, km_out["counts"].ctypes.data,
                        C.addressof(it), C.addressof(conv))
        api._call(api.lib().dinov2_hip_kmeans_tokens, s._h, C.byref(km))
        return {**km_out, "iterations": np.int32(it.value), "converged": np.int32(conv.value)}

    dev = lambda k: (lambda: s.predict_device(xd[k].ptr, B, h, w, classify=classify))
    c.step("predict", predict)
    c.step("layers", layers)
    c.step("attention", attention)
    c.step("layers_alone", layers_alone)
    c.step("dense", dense)
    c.step("dev_fetch", dev(0))
    c.step("fetch", fetch)
    c.step("dev_match", dev(1))
    c.step("match", match)
    c.step("dev_add", dev(0))
    c.step("bank_add", lambda: {"first": np.int32(bank.add(s, source="last_patches", image=1, n=P))})
    c.step("dev_topk", dev(1))
    c.step("bank_topk", bank_topk)
    c.step("dev_kmeans", dev(0))
    c.step("kmeans", kmeans)
    c.step("dev_pca", dev(1))
    c.step("pca3", lambda: dict(zip(("components", "mean", "projection"), s.pca3(None, shape=(P + (R if classify else 0), H)))))


def chain_G(c, classify=True):
    """predict_list_device with lists of different sizes and counts (work table and position cache are restaged), the second list once more
    in steady state with other images, and a host list behind a stall."""
    api, s = c.api, c.sess
    sizes1, sizes2 = [(56, 84), (28, 42), (70, 98)], [(28, 42), (70, 98), (70, 98), (56, 84)]
    hosts = {k: [images(1, hh, ww, 60 + 10 * k + i)[0] for i, (hh, ww) in enumerate(sz)] for k, sz in ((1, sizes1), (2, sizes2), (3, sizes2))}
    devs = {k: [c.upload("x%d_%d" % (k, i), a) for i, a in enumerate(v)] for k, v in hosts.items()}

    def outs(tag, sizes):
        rows = sum(patches(hh, ww) + (R if classify else 0) for hh, ww in sizes)
        kw = {"cls_ptr": c.dev(tag + ".cls", (len(sizes), H)).ptr, "patch_ptr": c.dev(tag + ".patch", (rows, H)).ptr}
        if classify:
            kw["logits_ptr"] = c.dev(tag + ".logits", (len(sizes), NCLS)).ptr
        return kw
    kw1, kw2, kw3 = outs("list1", sizes1), outs("list2", sizes2), outs("list2_again", sizes2)
    rows1 = sum(patches(hh, ww) + (R if classify else 0) for hh, ww in sizes1)
    lout = c.make("host_list_out", lambda: {"cls": stale_host(api, (3, H)), "patch_packed": stale_host(api, (rows1, H)),
                                            **({"logits": stale_host(api, (3, NCLS))} if classify else {})})
    c.step("list1", lambda: s.predict_list_device([d.ptr for d in devs[1]], sizes1, classify=classify, **kw1))
    c.step("list2", lambda: s.predict_list_device([d.ptr for d in devs[2]], sizes2, classify=classify, **kw2))
    c.step("list2_again", lambda: s.predict_list_device([d.ptr for d in devs[3]], sizes2, classify=classify, **kw3))

    def host_list():
        il, keep = api._image_list([a.ctypes.data for a in hosts[1]], sizes1, api.RGB_CHW, 0)
        o = api.Output()
        o.cls, o.patch_tokens = lout["cls"].ctypes.data, lout["patch_packed"].ctypes.data
        if classify:
            o.logits = lout["logits"].ctypes.data
        api._call(api.lib().dinov2_hip_predict_list, s._h, C.byref(il), C.byref(o), api.CLASSIFY if classify else 0)
        c.keep.append(keep)
        return lout
    c.step("host_list", host_list)


def chain_I(c, classify=True):
    """Host input with an asynchronous return, page-locked and pageable: device outputs, and out == NULL followed by fetch.  The input is
    left alone until the end, as the header asks; it gives the calm run's bits, and with page-locked input the call returns while the
    stream is busy."""
    api, s = c.api, c.sess
    B, h, w = 2, 56, 84
    xs = [images(B, h, w, 70 + k) for k in range(4)]

    def pinned(a):
        p = api.pinned_empty(a.shape)
        p[...] = a
        return p
    pin = c.make("pinned", lambda: [pinned(xs[0]), pinned(xs[2])])
    xw = c.upload("xw", images(B, h, w, 75))
    wkw = device_outputs(c, "warm", B, h, w, classify)
    o_pin, o_page = api._device_output(**_as_output(device_outputs(c, "pinned_dev", B, h, w, classify))), \
        api._device_output(**_as_output(device_outputs(c, "pageable_dev", B, h, w, classify)))
    f1, fo1 = c.make("fetch1", lambda: host_outputs(api, B, h, w, classify))
    f2, fo2 = c.make("fetch2", lambda: host_outputs(api, B, h, w, classify))

    def fetch(o, arrays):
        fetch_raw(api, s, o)
        return arrays
    c.step("warm", lambda: s.predict_device(xw.ptr, B, h, w, classify=classify, **wkw))
    c.step("pinned_dev", lambda: predict_raw(api, s, pin[0].ctypes.data, B, h, w, classify, o_pin, 0))
    c.step("pageable_dev", lambda: predict_raw(api, s, xs[1].ctypes.data, B, h, w, classify, o_page, 0))
    c.step("pinned_null", lambda: predict_raw(api, s, pin[1].ctypes.data, B, h, w, classify, None, 0))
    c.step("fetch_pinned", lambda: fetch(fo1, f1))
    c.step("pageable_null", lambda: predict_raw(api, s, xs[3].ctypes.data, B, h, w, classify, None, 0))
    c.step("fetch_pageable", lambda: fetch(fo2, f2))
    c.objects["keep_inputs"] = xs  # (pageable inputs stay alive and unchanged until the run is freed)


def _as_output(kw):
    """device_outputs' keywords under the parameter names of api._device_output."""
    return {"cls_ptr": kw.get("cls_ptr", 0), "patch_ptr": kw.get("patch_ptr", 0), "logits_ptr": kw.get("logits_ptr", 0),
            "probs_ptr": kw.get("probs_ptr", 0)}


# id -> (chain, fixture, ln_fold, classify, on a caller's stream)
SCENARIOS = {
    "A":          (chain_A, "tiny_gelu_reg4", 0, True, True),
    "A_features": (chain_A, "tiny_swiglu_reg4", 0, False, True),
    "B":          (chain_B, "tiny_swiglu_reg4", 0, True, False),
    "C_classify": (chain_C, "tiny_gelu_reg4", 0, True, False),
    "C_features": (chain_C, "tiny_swiglu_reg4", 0, False, False),
    "C_ln_fold":  (chain_C, "tiny_gelu_reg4", 1, True, False),
    "D":          (chain_D, "tiny_gelu_reg4", 0, True, False),
    "E":          (chain_E, "tiny_gelu_reg4", 0, True, False),
    "F":          (chain_F, "tiny_gelu_reg4", 0, True, False),
    "G":          (chain_G, "tiny_swiglu_reg4", 0, True, False),
    "I":          (chain_I, "tiny_gelu_reg4", 0, True, False),
}
GRAPH_SCENARIOS = ("A", "B", "C_classify")  # scenario J: these chains in a child process with DINOV2_HIP_GRAPHS=1
GRAPH_REPEATS = 4                           # first sighting eager, second captured, third and fourth replayed


def table_id(sid):
    return sid.split("_")[0]


def dry_steps(sid):
    """The step names of scenario `sid` in order, without a device."""
    chain, _, _, classify, _ = SCENARIOS[sid]
    c = Run(_DryApi(), table_id(sid), False, dry=True)
    chain(c, classify)
    return c.order


class _DryApi:
    """What a chain touches of the api module outside its steps."""
    CLASSIFY = 1

    @staticmethod
    def _device_output(**kw):
        return None

    @staticmethod
    def pinned_empty(shape):
        return np.empty(shape, np.float32)


_models = {}


def model_of(api, golden_dir, name, ln_fold):
    key = (name, ln_fold)
    if key not in _models:
        m = api.Model(os.path.join(golden_dir, name + ".gguf"), classify=True, ln_fold=ln_fold)
        hp = m.hparams
        assert (hp.hidden_size, hp.num_register_tokens, hp.num_classes, hp.patch_size, hp.num_attention_heads, hp.num_hidden_layers) == \
            (H, R, NCLS, PS, HEADS, LAYERS), "the tiny fixtures changed: tests/stream_cases.py states their sizes"
        _models[key] = m
    return _models[key]


def execute(api, golden_dir, sid, stalled, repeats=1):
    """One run of scenario `sid` on a fresh session: (results by name, {ASYNC step: [stream still busy on return, per repeat]})."""
    chain, fixture, ln_fold, classify, caller_stream = SCENARIOS[sid]
    model = model_of(api, golden_dir, fixture, ln_fold)
    S = api.Stream() if caller_stream else None
    sess = api.Session(model, stream=S.handle if S else None)
    stream = S or api.Stream(handle=sess.stream)
    run = Run(api, table_id(sid), stalled, sess, stream, model)
    try:
        for _ in range(repeats):
            chain(run, classify)
        res = run.finish()
        if caller_stream:
            assert sess.stream == S.handle, "the session does not report the stream it was given"
            sess.free()
            a, b = run.outputs["copy.patch"], run.outputs["out.patch"]
            a_before = a.to_host()
            S.copy(a, b)  # the caller's stream outlives the session and still works
            S.synchronize()
            assert S.query() and check_exact(a.to_host(), a_before, "copy on the caller's stream after session_free")[0]
    finally:
        sess.free()
        run.free()
        if S:
            S.destroy()
    return res, run.busy


def compare(calm, stalled, what):
    """[messages]: every output of every step, stalled against calm, bit for bit."""
    bad = []
    if set(calm) != set(stalled):
        bad.append(f"{what}: outputs {sorted(set(calm) ^ set(stalled))} in one run only")
    for k in sorted(set(calm) & set(stalled)):
        ok, msg = check_exact(stalled[k], calm[k], f"{what} {k} (stalled against calm)")
        if not ok:
            bad.append(msg)
        for mode, r in (("calm", calm), ("stalled", stalled)):
            if np.asarray(r[k]).dtype.kind == "f" and np.isnan(r[k]).any():
                bad.append(f"{what} {k}: the {mode} run left NaN behind")
    return bad


def not_busy(busy):
    """The ASYNC steps whose stream had drained when the call returned."""
    return sorted(k for k, v in busy.items() if not all(v))


# --------------------------------------------------------------------------------------------------------------- scenario H
def run_H(api, golden_dir):
    """Two sessions of one model on two caller streams, one stalled (by the op's longest stall) and one not: the free session's host results
    arrive, and are right, while the stalled stream is still busy; both are right at the end.  Returns (messages, busy flags)."""
    model = model_of(api, golden_dir, "tiny_gelu_reg4", 0)
    B, h, w = 2, 56, 84
    xa, xb = images(B, h, w, 80), images(B, h, w, 81)
    results = []
    for stalled in (False, True):
        S1, S2 = api.Stream(), api.Stream()
        s1, s2 = api.Session(model, stream=S1.handle), api.Session(model, stream=S2.handle)
        c = Run(api, "H", stalled, s1, S1, model)
        try:
            da = c.upload("xa", xa)
            kw, wkw = device_outputs(c, "stalled", B, h, w, True), device_outputs(c, "warm", B, h, w, True)
            free_out, fo = c.make("free_out", lambda: host_outputs(api, B, h, w, True))
            warm_out, wo = c.make("warm_out", lambda: host_outputs(api, B, h, w, True))

            def host(sess, x, o, arrays):
                predict_raw(api, sess, x.ctypes.data, B, h, w, True, o, 0)
                return arrays
            c.stalled = False  # both sessions see their shape first, calmly
            c.step("warm_stalled", lambda: s1.predict_device(da.ptr, B, h, w, classify=True, **wkw))
            c.step("warm_free", lambda: host(s2, xa, wo, warm_out), sess=s2, stream=S2)
            c.stalled = stalled
            if stalled:
                api.stream_delay(S1, 100 - STALL_MS)  # (step() adds STALL_MS: the op's cap in all)
            c.step("stalled", lambda: s1.predict_device(da.ptr, B, h, w, classify=True, **kw))
            c.stalled = False  # the free session's stream gets no stall
            c.step("free", lambda: host(s2, xb, fo, free_out), sess=s2, stream=S2)
            c.busy["free returned while the other stream was stalled"] = [not stalled or not S1.query()]
            results.append((c.finish((s1, s2)), dict(c.busy)))
        finally:
            s1.free()
            s2.free()
            c.free()
            S1.destroy()
            S2.destroy()
    (calm, _), (st, busy) = results
    return compare(calm, st, "H"), busy


# --------------------------------------------------------------------------------------------------------------- scenario K
def run_K(api, golden_dir):
    """A bank filled through one session behind a stall and searched, the moment bank_add has returned, through ANOTHER session on another
    stream: "a returned bank is always complete" holds for every session, not only on the stream that filled it -- the wait in bank_add, which no
    one-stream chain can see.  Returns (messages, busy flags)."""
    model = model_of(api, golden_dir, "tiny_gelu_reg4", 0)
    B, h, w = 2, 56, 84
    P = patches(h, w)
    xa, xb = images(B, h, w, 82), images(B, h, w, 83)
    results = []
    for stalled in (False, True):
        S1, S2 = api.Stream(), api.Stream()
        s1, s2 = api.Session(model, stream=S1.handle), api.Session(model, stream=S2.handle)
        c = Run(api, "K", stalled, s1, S1, model)
        try:
            da = c.upload("xa", xa)
            bank = c.make("bank", lambda: api.Bank(model, H, 2 * P))
            wkw = device_outputs(c, "warm", B, h, w, True)
            other, oo = c.make("other_out", lambda: host_outputs(api, B, h, w, True))
            found = c.make("topk_out", lambda: {"idx": stale_host(api, (B, 3), np.int32), "sim": stale_host(api, (B, 3))})

            def warm_other():
                predict_raw(api, s2, xb.ctypes.data, B, h, w, True, oo, 0)
                return other

            def topk_other():
                t = api.TopK(api.Rows(api.ROWS_LAST_CLS, None, B, H, 0, 0), 3, found["idx"].ctypes.data, found["sim"].ctypes.data)
                api._call(api.lib().dinov2_hip_bank_topk, s2._h, bank._h, C.byref(t))
                return found
            c.stalled = False
            c.step("warm", lambda: s1.predict_device(da.ptr, B, h, w, classify=True, **wkw))
            c.step("warm_other", warm_other, sess=s2, stream=S2)
            c.stalled = stalled
            c.step("forward", lambda: s1.predict_device(da.ptr, B, h, w, classify=True))
            c.step("bank_add", lambda: {"first": np.int32(bank.add(s1, source="last_patches", image=1, n=P))})
            c.stalled = False  # the searching session's stream gets no stall and no synchronisation before its call
            c.step("topk_other", topk_other, sess=s2, stream=S2)
            results.append((c.finish((s1, s2)), dict(c.busy)))
        finally:
            s1.free()
            s2.free()
            c.free()
            S1.destroy()
            S2.destroy()
    (calm, _), (st, busy) = results
    return compare(calm, st, "K"), busy


# --------------------------------------------------------------------------------------------------------------- scenario J
def child_main(golden_dir, out_path):
    """In a child process started with DINOV2_HIP_GRAPHS=1: the stalled runs of GRAPH_SCENARIOS, each chain GRAPH_REPEATS times on one
    session so that captured graphs are replayed; results to `out_path`, one line per scenario with the steps that were not busy."""
    from importlib import import_module
    from __graft_entry__ import PKG_NAME, load_package
    load_package()
    api = import_module(PKG_NAME + ".api")
    out = {}
    for sid in GRAPH_SCENARIOS:
        res, busy = execute(api, golden_dir, sid, True, GRAPH_REPEATS)
        out.update({sid + "/" + k: v for k, v in res.items()})
        print("NOT_BUSY", sid, ",".join(not_busy(busy)) or "-")
    np.savez(out_path, **out)
    print("STREAMS_OK")
