"""The per-step glue kernels per element against the float64 references and bounds of tests/glue_cases.py (proved on the CPU by
tests/test_glue_cases_host.py): csrc/elementwise.hip, csrc/elementwise_bf16.hip, rn_wino_weights / rn_wino_dw of csrc/conv_wino.hip and
csrc/optim.hip, at the shapes where their index arithmetic can go wrong.

Every entry point is called through the C ABI (ctypes), not through the allocating wrappers of conv.py, so that the test owns every
buffer: each output starts as NaN (floats) or all-ones bytes and is 64 bytes longer than the kernel may write, and "wrote every element
it owns and nothing else" is part of each comparison; padded input slots hold NaN, so a read of one shows in the result.  A comparison is
bit-equality or gc.within(result, reference, bound); the largest error seen in each family, as a fraction of its bound, is printed when
the module finishes (run with -s to see the lines): information, not a threshold.

Entry point -> the test that calls it:
  rn_pack_weights             test_pack, test_prep_batched
  rn_bn_fold                  test_fold
  rn_wino_weights             test_wino_weights
  rn_prep_batched             test_prep_batched, test_engine_tables (through Engine._prepare_training)
  rn_unpack_wgrad             test_unpack, test_unpack_batched
  rn_unpack_batched           test_unpack_batched
  rn_wino_dw                  test_wino_dw
  rn_maxpool_fwd              test_pool_forward
  rn_maxpool_fwd_bf16out      test_pool_forward
  rn_maxpool_bwd              test_pool_backward
  rn_maxpool_bwd_bf16in       test_pool_backward
  rn_upsample_add_bwd         test_upsample_add_bwd
  rn_upsample_add_bwd_bf16    test_upsample_add_bwd
  rn_sigmoid_bwd_pad          test_sigmoid_bwd_pad, test_sigmoid_bwd_pad_flags
  rn_sigmoid_bwd_pad_bf16     test_sigmoid_bwd_pad
  rn_sigmoid_bwd_pad_flags    test_sigmoid_bwd_pad_flags
  rn_colsum_workspace_bytes   test_colsum
  rn_colsum                   test_colsum
  rn_relu_mask                test_relu_mask
  rn_relu_bf16                test_relu_bf16
  rn_add_inplace              test_add_inplace
  rn_nchw_to_nhwc4            test_nchw_to_nhwc4
  rn_opt_clip_adam_hp         test_clip_adam_past_1024_chunks (through ClipAdam.step, which makes that one call)
(rn_split_weights, rn_split_weights_f16 and rn_f32_to_bf16 of other files are the single-call twins test_prep_batched compares kinds 3,
4 and 5 with.)"""
import numpy as np
import pytest
import torch

import glue_cases as gc

pytestmark = pytest.mark.gpu

RN_EINVAL = 10001
GUARD = 64                                # bytes behind every output that must keep their poison
WORST = {}                                # family -> largest error seen, as a fraction of its bound


@pytest.fixture(scope="module")
def lib(dev):
    from retinanet_mi355x import _hip
    yield _hip.load()
    PASSED.clear()
    lines = ["glue %-28s worst error %.3f of its bound" % (k, v) for k, v in sorted(WORST.items())]
    print("\n" + "\n".join(lines))


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """A kernel fault poisons the context: end the session there, start nothing more on the device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, stopping: %s" % e, returncode=3)


def st():
    return torch.cuda.current_stream().cuda_stream


def bounded(family, got, ref, bound):
    """gc.within, with the fraction noted for the module's report."""
    w = gc.worst(got, ref, bound)
    WORST[family] = max(WORST.get(family, 0.0), w)
    assert w <= 1.0, "%s: error %.3f of its bound" % (family, w)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Out:
    """An output buffer of `n` elements of `dtype`, all-ones bytes (NaN for fp32 and bf16), with GUARD bytes behind it."""

    def __init__(self, n, dev, dtype=np.float32):
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.buf = torch.full((self.n * self.dtype.itemsize + GUARD,), 255, dtype=torch.uint8, device=dev)

    def ptr(self):
        return self.buf.data_ptr()

    def get(self, shape=None):
        """The owned elements; the guard must be untouched."""
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        assert (raw[self.n * self.dtype.itemsize:] == 255).all(), "the bytes behind the output were written"
        a = raw[:self.n * self.dtype.itemsize].view(self.dtype)
        return a if shape is None else a.reshape(shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == 255).all())


def bf16_dev(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def table(structs, dev):
    arr = (type(structs[0]) * len(structs))(*structs)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def shuffled(chunks, seed, dev):
    """Chunk rows in a seeded random order (not sorted by job)."""
    order = torch.randperm(len(chunks), generator=torch.Generator().manual_seed(seed)).tolist()
    assert order != sorted(order)
    return torch.tensor([chunks[i] for i in order], dtype=torch.int32).to(dev)


# ---------------------------------------------------------------------------------------------- 1. weight preparation
def pack_call(lib, c, w, scale, dst_ptr):
    r0, nr, s0, ns = c.taps if c.taps is not None else (0, 0, 0, 0)
    return lib.rn_pack_weights(w.data_ptr(), dst_ptr, c.cout, c.cin, c.kh, c.kw, c.kw_pad, c.c_pad, c.mode,
                               None if scale is None else scale.data_ptr(), r0, nr, s0, ns, st())


@pytest.mark.parametrize("c", gc.PACK, ids=lambda c: c.name)
def test_pack(lib, dev, c):
    """A pack is a copy (one fp32 product with scale): bit-equal, padding exactly +0.0."""
    w, scale = gc.pack_inputs(c)
    want = gc.pack_ref(w, c.kw_pad, c.c_pad, c.mode, scale, c.taps)
    out = Out(want.size, dev)
    wg, sg = up(w, dev), None if scale is None else up(scale, dev)
    assert pack_call(lib, c, wg, sg, out.ptr()) == 0
    assert gc.same_bits(out.get(want.shape), want)


@pytest.mark.parametrize("C", gc.FOLD_C)
def test_fold(lib, dev, C):
    ins = gc.fold_inputs(C)
    (rstd, scale, shift), (b_rstd, b_scale, b_shift) = gc.fold_ref(*ins)
    g = [up(a, dev) for a in ins]
    o_scale, o_shift, o_rstd = Out(C, dev), Out(C, dev), Out(C, dev)
    assert lib.rn_bn_fold(g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), gc.FOLD_EPS, C, o_scale.ptr(), o_shift.ptr(),
                          o_rstd.ptr(), st()) == 0
    bounded("fold rstd", o_rstd.get(), rstd, b_rstd)
    bounded("fold scale", o_scale.get(), scale, b_scale)
    bounded("fold shift", o_shift.get(), shift, b_shift)
    # without rstd the other two are the same
    o2, o3 = Out(C, dev), Out(C, dev)
    assert lib.rn_bn_fold(g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), gc.FOLD_EPS, C, o2.ptr(), o3.ptr(), None, st()) == 0
    assert gc.same_bits(o2.get(), o_scale.get()) and gc.same_bits(o3.get(), o_shift.get())


@pytest.mark.parametrize("cout,cin", gc.WINO_W)
@pytest.mark.parametrize("mode,scaled", [(0, False), (1, True), (1, False)])
def test_wino_weights(lib, dev, cout, cin, mode, scaled):
    w, scale = gc.wino_w_inputs(cout, cin)
    ref, bound = gc.wino_weights_ref(w, mode, scale if scaled else None)
    out = Out(ref.size, dev)
    wg, sg = up(w, dev), up(scale, dev)
    assert lib.rn_wino_weights(wg.data_ptr(), out.ptr(), cout, cin, mode, sg.data_ptr() if scaled else None, st()) == 0
    bounded("wino weights", out.get(ref.shape), ref, bound)


def test_prep_batched(lib, dev):
    """One launch over hand-built jobs of every kind 0 .. 5 with the chunk rows shuffled: kinds 1, 3, 4, 5 bit-equal to the single-call
    entry points on the same input, kinds 0 and 2 inside the single calls' float64 bounds, every byte outside a job's own all-ones."""
    from retinanet_mi355x import _hip, conv as cv
    jobs, chunks, checks, keep = [], [], [], []

    def add(j, blocks):
        chunks.extend((len(jobs), b) for b in range(blocks))
        jobs.append(j)

    # kind 0: folds of 255 and 257 channels (one chunk, two chunks)
    for C in (255, 257):
        ins = gc.fold_inputs(C)
        g = [up(a, dev) for a in ins]
        outs = [Out(C, dev) for _ in range(3)]
        keep += g
        j = _hip.PrepJob()
        j.kind, j.Cout, j.eps = 0, C, gc.FOLD_EPS
        j.gamma, j.beta, j.mean, j.var = (t.data_ptr() for t in g)
        j.bn_scale, j.bn_shift, j.bn_rstd = (o.ptr() for o in outs)
        add(j, gc.prep_blocks(0, Cout=C))
        (rstd, scale, shift), (b_rstd, b_scale, b_shift) = gc.fold_ref(*ins)
        checks.append(lambda outs=outs, r=(scale, shift, rstd), b=(b_scale, b_shift, b_rstd): [
            bounded("prep_batched fold", o.get(), rr, bb) for o, rr, bb in zip(outs, r, b)])
    # kind 1: every pack case
    for c in gc.PACK:
        w, scale = gc.pack_inputs(c)
        want = gc.pack_ref(w, c.kw_pad, c.c_pad, c.mode, scale, c.taps)
        wg, sg = up(w, dev), None if scale is None else up(scale, dev)
        keep += [wg, sg]
        out, single = Out(want.size, dev), Out(want.size, dev)
        assert pack_call(lib, c, wg, sg, single.ptr()) == 0
        j = _hip.PrepJob()
        j.kind, j.Cout, j.Cin, j.kh, j.kw, j.kw_pad, j.c_pad, j.mode = 1, c.cout, c.cin, c.kh, c.kw, c.kw_pad, c.c_pad, c.mode
        j.r0, j.nr, j.s0, j.ns = c.taps if c.taps is not None else (0, 0, 0, 0)
        j.rows, j.Kpad = want.shape
        j.src, j.dst, j.scale = wg.data_ptr(), out.ptr(), None if sg is None else sg.data_ptr()
        add(j, gc.prep_blocks(1, rows=want.shape[0], Kpad=want.shape[1]))
        checks.append(lambda out=out, single=single, want=want: (gc.same_bits(out.get(), single.get()) and gc.same_bits(out.get(want.shape), want))
                      or pytest.fail("kind 1 differs from rn_pack_weights"))
    # kind 2: the Winograd transform, both cases, mode 0 and mode 1 with and without scale
    for cout, cin in gc.WINO_W:
        w, scale = gc.wino_w_inputs(cout, cin)
        wg, sg = up(w, dev), up(scale, dev)
        keep += [wg, sg]
        for mode, scaled in ((0, False), (1, True), (1, False)):
            ref, bound = gc.wino_weights_ref(w, mode, scale if scaled else None)
            out = Out(ref.size, dev)
            j = _hip.PrepJob()
            j.kind, j.Cout, j.Cin, j.mode = 2, cout, cin, mode
            j.rows, j.Kpad = ref.shape[1], ref.shape[2]
            j.src, j.dst, j.scale = wg.data_ptr(), out.ptr(), sg.data_ptr() if scaled else None
            add(j, gc.prep_blocks(2, rows=ref.shape[1], Kpad=ref.shape[2]))
            checks.append(lambda out=out, ref=ref, bound=bound: bounded("prep_batched wino weights", out.get(ref.shape), ref, bound))
    # kinds 3, 4, 5 read an already packed fp32 buffer: sources of their own (in the engine they run one launch after what fills them)
    def packed(rows, Kpad, seed):
        t = up(gc.synth.normal((rows, Kpad), seed), dev)
        keep.append(t)
        return t

    for rows, Kpad, seed in ((7, 32, 400), (5, 224, 401)):                      # kind 3: bf16 cast, one chunk and five
        src = packed(rows, Kpad, seed)
        out = Out(rows * Kpad, dev, np.uint16)
        j = _hip.PrepJob()
        j.kind, j.rows, j.Kpad, j.src, j.dst = 3, rows, Kpad, src.data_ptr(), out.ptr()
        add(j, gc.prep_blocks(3, rows=rows, Kpad=Kpad))

        def check3(out=out, src=src):
            want = src.to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)
            assert gc.same_bits(out.get(), want), "kind 3 differs from tensor.to(torch.bfloat16)"
            assert gc.same_bits(out.get(), cv.to_bf16(src).view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1))
            assert gc.same_bits(out.get(), gc.bf16_rne(src.cpu().numpy()).reshape(-1))
        checks.append(check3)
    for shape, seed in (((6, 96), 402), ((36, 5, 32), 403)):                    # kind 4: a 2-D pack and a 3-D Winograd U (rows = 36 Cout)
        Kpad = shape[-1]
        rows = int(np.prod(shape[:-1]))
        src = packed(rows, Kpad, seed).view(shape)
        out, single = Out(rows * Kpad * 6, dev, np.uint8), Out(rows * Kpad * 6, dev, np.uint8)
        assert lib.rn_split_weights(src.data_ptr(), single.ptr(), rows, Kpad, st()) == 0
        j = _hip.PrepJob()
        j.kind, j.rows, j.Kpad, j.src, j.dst = 4, rows, Kpad, src.data_ptr(), out.ptr()
        add(j, gc.prep_blocks(4, rows=rows, Kpad=Kpad))
        checks.append(lambda out=out, single=single: gc.same_bits(out.get(), single.get()) or pytest.fail("kind 4 differs from rn_split_weights"))
    for rows, Kpad, seed in ((1, 32, 404), (5, 96, 405)):                       # kind 5: row counts that are no multiples of 4
        src = packed(rows, Kpad, seed)
        outs = [Out(rows * Kpad * 4, dev, np.uint8), Out(rows, dev)]
        singles = [Out(rows * Kpad * 4, dev, np.uint8), Out(rows, dev)]
        assert lib.rn_split_weights_f16(src.data_ptr(), singles[0].ptr(), singles[1].ptr(), rows, Kpad, st()) == 0
        j = _hip.PrepJob()
        j.kind, j.rows, j.Kpad, j.src, j.dst, j.bn_scale = 5, rows, Kpad, src.data_ptr(), outs[0].ptr(), outs[1].ptr()
        add(j, gc.prep_blocks(5, rows=rows, Kpad=Kpad))
        checks.append(lambda outs=outs, singles=singles: all(gc.same_bits(o.get(), s.get()) for o, s in zip(outs, singles))
                      or pytest.fail("kind 5 differs from rn_split_weights_f16"))
    assert sorted({j.kind for j in jobs}) == [0, 1, 2, 3, 4, 5]
    jt, ct = table(jobs, dev), shuffled(chunks, 7, dev)
    assert lib.rn_prep_batched(jt.data_ptr(), ct.data_ptr(), len(chunks), st()) == 0
    torch.cuda.synchronize()
    for check in checks:
        check()


PASSED = {}                               # (layer, buffer) -> a device tensor that has met its float64 bound


def bounded_once(key, family, t, reference):
    """bounded(t, *reference()), unless t is bit for bit a tensor that already met that bound: the folds and the Winograd transforms do not
    depend on the product mode, so the second and third mode of test_engine_tables find the first one's buffers again (the parameters are the
    same) and are spared the float64 work; anything else is compared in full."""
    seen = PASSED.get(key)
    if seen is not None and same_tensor_bits(seen, t):
        return
    bounded(family, t.cpu().numpy(), *reference())
    PASSED[key] = t.clone()


def int_bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def same_tensor_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(int_bits(a), int_bits(b))


@pytest.mark.parametrize("mode", ["native", "split", "split3"])
def test_engine_tables(lib, dev, mode):
    """Engine._build_prep's tables (chunk counts per kind, which launch a job goes into) on ResNet-18: after _prepare_training every
    layer's adopted buffers equal what the per-call builders make of the same parameters -- bit for bit, or inside the float64 bound for
    the fold and the Winograd transform -- with every destination poisoned between two runs of the tables, so that an element the tables
    do not cover shows.  (The bf16 twins wf16 / wd16 belong to the bottleneck networks' engines and are left to kind 3 above.)"""
    from retinanet_mi355x import arch, conv as cv, modules, synth
    before = cv.get_fp32_mfma(), cv.PRESPLIT
    cv.set_fp32_mfma(mode)
    cv.PRESPLIT = mode != "native"
    try:
        sd = synth.state_dict("resnet18", num_classes=4, n_reg=12, seed=7, head_scale=3e-4)
        net = modules.resnet18(num_classes=4)
        net.load_state_dict(sd)
        net = net.to(dev)
        eng, P = net._engine, net._tensor_dict()
        eng._prepare_training(P)                     # builds the tables
        twins = 0

        def tensors(b):
            for v in b.values():
                for t in (v if isinstance(v, (list, tuple)) else [v]):
                    yield t
                    for name in ("_rn_split", "_rn_split16"):
                        tw = getattr(t, name, None)
                        yield from ([] if tw is None else tw if isinstance(tw, tuple) else [tw])
        for b in eng._prep["bufs"].values():
            for t in tensors(b):
                t.view(-1).view(torch.uint8).fill_(255)
        eng._prepare_training(P)                     # the same tables again, over poisoned destinations
        torch.cuda.synchronize()
        min_k = lib.rn_fp32_split_min_k()

        def check_twins(buf, what):
            nonlocal twins
            ws, ws16 = getattr(buf, "_rn_split", None), getattr(buf, "_rn_split16", None)
            if mode == "native" or buf.shape[-1] < min_k:
                assert ws is None and ws16 is None, what
                return
            fresh = buf.clone()
            if mode == "split3":
                assert ws is None and ws16 is not None, what
                cv.split_weights_f16(fresh)
                assert same_tensor_bits(ws16[0], fresh._rn_split16[0]) and same_tensor_bits(ws16[1], fresh._rn_split16[1]), what
            else:
                assert ws16 is None and ws is not None, what
                cv.split_weights(fresh)
                assert same_tensor_bits(ws, fresh._rn_split), what
            twins += 1

        n_wino = n_classes = 0
        for name, L in eng.layers.items():
            s = L.spec
            w = P[s.name + ".weight"]
            assert same_tensor_bits(L.wf, cv.pack_weights(w, 0, kw_pad=L.kw_pad, c_pad=L.cin_pad, presplit=False)), name
            check_twins(L.wf, name + " wf")
            if s.bn:
                ins = [P[s.bn + k].detach().cpu().numpy() for k in (".weight", ".bias", ".running_mean", ".running_var")]
                (rstd, scale, shift), (b_rstd, b_scale, b_shift) = gc.fold_ref(*ins, eps=arch.BN_EPS)
                bounded_once((name, "rstd"), "engine fold", L.rstd, lambda: (rstd, b_rstd))
                bounded_once((name, "scale"), "engine fold", L.scale, lambda: (scale, b_scale))
                bounded_once((name, "shift"), "engine fold", L.shift, lambda: (shift, b_shift))
            else:
                assert L.scale is None and L.rstd is None
            if eng.use_wino and L.wino_layer:
                n_wino += 1
                assert L.wd is None and L.uf is not None and L.ud is not None
                wn = w.detach().cpu().numpy()
                sc = None if L.scale is None else L.scale.cpu().numpy()
                bounded_once((name, "uf"), "engine wino weights", L.uf, lambda: gc.wino_weights_ref(wn, 0))
                bounded_once((name, "ud", sc is None), "engine wino weights", L.ud, lambda: gc.wino_weights_ref(wn, 1, sc))
                check_twins(L.uf, name + " uf")
                check_twins(L.ud, name + " ud")
                continue
            assert L.uf is None and L.ud is None
            if name == "conv1":
                assert L.wd is None
            elif s.stride == 2 and s.k > 1:
                classes = cv.s2_classes(s.k, s.pad)
                assert isinstance(L.wd, list) and len(L.wd) == len(classes) == 4
                for d, c in zip(L.wd, classes):
                    assert same_tensor_bits(d, cv.pack_weights(w, 1, scale=L.scale, c_pad=L.cout_pad, taps=c[2], presplit=False)), name
                    check_twins(d, name + " wd class")
                n_classes += 1
            else:
                assert same_tensor_bits(L.wd, cv.pack_weights(w, 1, scale=L.scale, kw_pad=s.k, c_pad=L.cout_pad, presplit=False)), name
                check_twins(L.wd, name + " wd")
        assert n_wino >= 8 and n_classes >= 3 and (twins > 0) == (mode != "native"), (n_wino, n_classes, twins)
    finally:
        cv.set_fp32_mfma(before[0])
        cv.PRESPLIT = before[1]


# ---------------------------------------------------------------------------------------------- 2. weight-gradient unpack
def unpack_operands(d, dev):
    return {k: up(d[k], dev) for k in ("dw", "wp", "scale", "mean", "rstd", "colsum")}


def unpack_pointers(form, g):
    """(w_packed, scale, mean, rstd, colsum) of a form: batch norm; bias (dbeta only); neither."""
    p = lambda k: g[k].data_ptr()
    if form == "bn":
        return p("wp"), p("scale"), p("mean"), p("rstd"), p("colsum")
    return None, None, None, None, (p("colsum") if form == "bias" else None)


def unpack_check(c, form, d, dweight, dgamma, dbeta, family):
    n = c.cin * c.kh * c.kw
    want, ref_gamma, bound = gc.unpack_ref(d, scaled=form == "bn")
    got = dweight.get((c.cout, n))
    assert np.isfinite(got).all(), "a padded slot of dw was read"
    assert gc.same_bits(got, want)
    if form == "bn":
        bounded(family, dgamma.get(), ref_gamma, bound)
    else:
        assert dgamma.untouched()
    if form == "plain":
        assert dbeta.untouched()
    else:
        assert gc.same_bits(dbeta.get(), d["colsum"])


@pytest.mark.parametrize("form", gc.UNPACK_FORMS)
@pytest.mark.parametrize("c", gc.UNPACK, ids=lambda c: c.name)
def test_unpack(lib, dev, c, form):
    d = gc.unpack_inputs(c)
    g = unpack_operands(d, dev)
    n = c.cin * c.kh * c.kw
    dweight, dgamma, dbeta = Out(c.cout * n, dev), Out(c.cout, dev), Out(c.cout, dev)
    wp, scale, mean, rstd, colsum = unpack_pointers(form, g)
    assert lib.rn_unpack_wgrad(g["dw"].data_ptr(), wp, dweight.ptr(), c.cout, c.cin, c.kh, c.kw, c.kw_pad, c.c_pad, scale, mean, rstd, colsum,
                               dgamma.ptr() if form == "bn" else None, dbeta.ptr() if form != "plain" else None, st()) == 0
    unpack_check(c, form, d, dweight, dgamma, dbeta, "unpack dgamma")


def test_unpack_batched(lib, dev):
    """The three shapes in the three forms as nine jobs of one launch, chunk rows (job, output channel) shuffled."""
    from retinanet_mi355x import _hip
    jobs, chunks, outs, keep = [], [], [], []
    for c in gc.UNPACK_BATCHED:
        d = gc.unpack_inputs(c)
        g = unpack_operands(d, dev)
        keep.append(g)
        n = c.cin * c.kh * c.kw
        for form in gc.UNPACK_FORMS:
            o = (Out(c.cout * n, dev), Out(c.cout, dev), Out(c.cout, dev))
            j = _hip.UnpackJob()
            j.dw, j.dweight = g["dw"].data_ptr(), o[0].ptr()
            j.w_packed, j.scale, j.mean, j.rstd, j.colsum = unpack_pointers(form, g)
            j.Cout, j.Cin, j.kh, j.kw, j.kw_pad, j.c_pad, j.Kpad = c.cout, c.cin, c.kh, c.kw, c.kw_pad, c.c_pad, d["dw"].shape[1]
            j.dgamma, j.dbeta = o[1].ptr() if form == "bn" else None, o[2].ptr() if form != "plain" else None
            chunks.extend((len(jobs), co) for co in range(c.cout))
            jobs.append(j)
            outs.append((c, form, d, o))
    jt, ct = table(jobs, dev), shuffled(chunks, 11, dev)
    assert lib.rn_unpack_batched(jt.data_ptr(), ct.data_ptr(), len(chunks), st()) == 0
    for (c, form, d, o), g in zip(outs, [g for g in keep for _ in gc.UNPACK_FORMS]):
        unpack_check(c, form, d, *o, "unpack_batched dgamma")
        # ... and bit-equal to the single launch
        n = c.cin * c.kh * c.kw
        s = (Out(c.cout * n, dev), Out(c.cout, dev), Out(c.cout, dev))
        wp, scale, mean, rstd, colsum = unpack_pointers(form, g)
        assert lib.rn_unpack_wgrad(g["dw"].data_ptr(), wp, s[0].ptr(), c.cout, c.cin, c.kh, c.kw, c.kw_pad, c.c_pad, scale, mean, rstd, colsum,
                                   s[1].ptr() if form == "bn" else None, s[2].ptr() if form != "plain" else None, st()) == 0
        assert gc.same_bits(o[0].get(), s[0].get()) and gc.same_bits(o[2].get(), s[2].get())


@pytest.mark.parametrize("cout,cin", gc.WINO_DW)
def test_wino_dw(lib, dev, cout, cin):
    dU, dw = gc.wino_dw_inputs(cout, cin)
    ref, bound = gc.wino_dw_ref(dU, dw, cin)
    dUg, dwg = up(dU, dev), up(dw, dev)
    assert lib.rn_wino_dw(dUg.data_ptr(), dwg.data_ptr(), cout, cin, st()) == 0
    got = dwg.cpu().numpy()
    assert np.isfinite(got[:, :9 * cin]).all(), "a column ci >= Cin of dU was read"
    bounded("wino dw", got[:, :9 * cin], ref, bound)
    assert gc.same_bits(got[:, 9 * cin:], dw[:, 9 * cin:]), "positions past 9 Cin were written"


# ---------------------------------------------------------------------------------------------- 3. pools
@pytest.mark.parametrize("shape", gc.POOL, ids=str)
def test_pool_forward(lib, dev, shape):
    N, C, H, W = shape
    Ho, Wo = gc.pool_out(H), gc.pool_out(W)
    x = gc.pool_x(shape)
    y_ref, a_ref = gc.pool_ref(x)
    xg = up(x, dev)
    y, arg, y_only = Out(y_ref.size, dev), Out(a_ref.size, dev, np.uint8), Out(y_ref.size, dev)
    assert lib.rn_maxpool_fwd(xg.data_ptr(), y.ptr(), arg.ptr(), N, H, W, C, Ho, Wo, st()) == 0
    assert lib.rn_maxpool_fwd(xg.data_ptr(), y_only.ptr(), None, N, H, W, C, Ho, Wo, st()) == 0
    assert gc.same_bits(y.get(y_ref.shape), y_ref) and gc.same_bits(arg.get(a_ref.shape), a_ref)
    assert gc.same_bits(y_only.get(y_ref.shape), y_ref)
    # bf16 result: the RNE rounding of the maximum, on the tied table and on values bf16 cannot hold; the same argmax as the fp32 kernel
    for xv in (x, gc.pool_x(shape, fine=True)):
        yv, av = gc.pool_ref(xv)
        xg = up(xv, dev)
        yb, ab, a32, y32 = Out(yv.size, dev, np.uint16), Out(av.size, dev, np.uint8), Out(av.size, dev, np.uint8), Out(yv.size, dev)
        assert lib.rn_maxpool_fwd_bf16out(xg.data_ptr(), yb.ptr(), ab.ptr(), N, H, W, C, Ho, Wo, st()) == 0
        assert lib.rn_maxpool_fwd(xg.data_ptr(), y32.ptr(), a32.ptr(), N, H, W, C, Ho, Wo, st()) == 0
        assert gc.same_bits(yb.get(yv.shape), gc.bf16_rne(yv))
        assert gc.same_bits(ab.get(), a32.get()) and gc.same_bits(ab.get(av.shape), av)
        yb2 = Out(yv.size, dev, np.uint16)
        assert lib.rn_maxpool_fwd_bf16out(xg.data_ptr(), yb2.ptr(), None, N, H, W, C, Ho, Wo, st()) == 0
        assert gc.same_bits(yb2.get(), yb.get())


@pytest.mark.parametrize("relu_mask", [0, 1, 2])
@pytest.mark.parametrize("shape", gc.POOL, ids=str)
def test_pool_backward(lib, dev, shape, relu_mask):
    """fp32 and bf16 gradients through the reference's argmax; mask 1 reads x (x > 0 is false for -0.0 and 0), mask 2 its sign bits
    (whole 32-channel groups only: every other channel count is refused and nothing is written)."""
    N, C, H, W = shape
    Ho, Wo = gc.pool_out(H), gc.pool_out(W)
    x = gc.pool_x(shape)
    _, arg = gc.pool_ref(x)
    dy = gc.synth.normal(arg.shape, 230)
    dyb = gc.bf16_rne(dy)
    xg, ag, dyg, dybg = up(x, dev), up(arg, dev), up(dy, dev), bf16_dev(dyb, dev)
    dx, dxb = Out(x.size, dev), Out(x.size, dev)
    if relu_mask == 2 and C % 32:
        words = torch.zeros(x.size // 32 + 1, dtype=torch.int32, device=dev)
        assert lib.rn_maxpool_bwd(words.data_ptr(), dyg.data_ptr(), ag.data_ptr(), dx.ptr(), N, H, W, C, Ho, Wo, 2, None, st()) == RN_EINVAL
        assert lib.rn_maxpool_bwd_bf16in(words.data_ptr(), dybg.data_ptr(), ag.data_ptr(), dxb.ptr(), N, H, W, C, Ho, Wo, 2, st()) == RN_EINVAL
        assert dx.untouched() and dxb.untouched()
        return
    mask = up(gc.sign_words(x).view(np.int32), dev) if relu_mask == 2 else xg
    keep = (x > 0) if relu_mask else None
    assert lib.rn_maxpool_bwd(mask.data_ptr(), dyg.data_ptr(), ag.data_ptr(), dx.ptr(), N, H, W, C, Ho, Wo, relu_mask, None, st()) == 0
    assert lib.rn_maxpool_bwd_bf16in(mask.data_ptr(), dybg.data_ptr(), ag.data_ptr(), dxb.ptr(), N, H, W, C, Ho, Wo, relu_mask, st()) == 0
    bounded("maxpool backward", dx.get(x.shape), *gc.pool_bwd_ref(arg, dy, H, W, keep))
    bounded("maxpool backward bf16 dy", dxb.get(x.shape), *gc.pool_bwd_ref(arg, gc.bf16_value(dyb), H, W, keep))


# ---------------------------------------------------------------------------------------------- 4. FPN, head, small elementwise
def guarded_inout(a, dev, dtype=np.float32):
    """An in/out buffer holding `a` with the all-ones guard behind it."""
    o = Out(a.size, dev, dtype)
    o.buf[:a.size * o.dtype.itemsize] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to(dev)
    return o


@pytest.mark.parametrize("C", gc.UPSAMPLE_C)
@pytest.mark.parametrize("case", gc.UPSAMPLE, ids=str)
def test_upsample_add_bwd(lib, dev, case, C):
    (Hs, Ws), (Hd, Wd) = case
    src, dst = gc.upsample_inputs(case, C)
    ref, bound = gc.upsample_add_bwd_ref(src, dst)
    sg, dg = guarded_inout(src, dev), guarded_inout(dst, dev)
    assert lib.rn_upsample_add_bwd(sg.ptr(), dg.ptr(), gc.UPSAMPLE_N, Hs, Ws, Hd, Wd, C, None, st()) == 0
    bounded("upsample_add_bwd", dg.get(dst.shape), ref, bound)
    src, dst = gc.upsample_inputs(case, C, bf16=True)
    ref, bound = gc.upsample_add_bwd_ref(src, dst, bf16=True)
    sg, dg = guarded_inout(gc.bf16_rne(src), dev, np.uint16), guarded_inout(gc.bf16_rne(dst), dev, np.uint16)
    assert lib.rn_upsample_add_bwd_bf16(sg.ptr(), dg.ptr(), gc.UPSAMPLE_N, Hs, Ws, Hd, Wd, C, st()) == 0
    bounded("upsample_add_bwd bf16", gc.bf16_value(dg.get(dst.shape)), ref, bound)


@pytest.mark.parametrize("with_s", [True, False])
@pytest.mark.parametrize("C,ld", gc.SIGMOID)
def test_sigmoid_bwd_pad(lib, dev, C, ld, with_s):
    """The source is a level's slice of a wider concatenated tensor (batch stride > rows * C, pointer offset into it, NaN around it)."""
    B, rows = gc.SIGMOID_B, gc.SIGMOID_ROWS
    whole, dy, off, stride = gc.concat_slice(B, rows, C, 17)
    gc.signed_zeros(dy)
    whole[:, off // C:off // C + rows] = dy
    s = gc.sigmoid_values((B, rows, C), 18)
    s_whole = np.full_like(whole, np.nan)
    s_whole[:, off // C:off // C + rows] = s
    wg, swg = up(whole, dev), up(s_whole, dev)
    sp = swg.data_ptr() + 4 * off if with_s else None
    ref, bound = gc.sigmoid_bwd_pad_ref(dy, s if with_s else None, ld)
    out = Out(ref.size, dev)
    assert lib.rn_sigmoid_bwd_pad(wg.data_ptr() + 4 * off, sp, out.ptr(), B, rows, C, ld, stride, None, st()) == 0
    bounded("sigmoid_bwd_pad", out.get(ref.shape), ref, bound)
    ref, bound = gc.sigmoid_bwd_pad_ref(dy, s if with_s else None, ld, bf16=True)
    outb = Out(ref.size, dev, np.uint16)
    assert lib.rn_sigmoid_bwd_pad_bf16(wg.data_ptr() + 4 * off, sp, outb.ptr(), B, rows, C, ld, stride, st()) == 0
    bounded("sigmoid_bwd_pad bf16", gc.bf16_value(outb.get(ref.shape)), ref, bound)
    # the bf16 result is the RNE rounding of the fp32 kernel's (same arithmetic, one more rounding)
    assert gc.same_bits(outb.get(), gc.bf16_rne(out.get()))


@pytest.mark.parametrize("with_s", [True, False])
@pytest.mark.parametrize("H,W,extra", [(9, 6, False), (4, 4, True)])
def test_sigmoid_bwd_pad_flags(lib, dev, H, W, extra, with_s):
    """One image per pixel position, so that no neighbour covers for a missing halo flag; (4, 4) is one tile per image, with an empty
    image after each, so that a write to a neighbouring flag lands on a byte that must stay 0."""
    C, ld = 5, 8
    dy, s, pixels = gc.flags_inputs(H, W, C, extra_empty=extra)
    if not with_s:
        pixels = pixels[:-1] + [(H - 1, W - 1)]            # without s the last image's value is not multiplied away
    B, TH, TW = len(pixels), (H + 3) // 4, (W + 3) // 4
    whole, _, off, stride = gc.concat_slice(B, H * W, C, 19)
    whole[:, off // C:off // C + H * W] = dy
    s_whole = np.full_like(whole, np.nan)
    s_whole[:, off // C:off // C + H * W] = s
    wg, swg = up(whole, dev), up(s_whole, dev)
    sp = swg.data_ptr() + 4 * off if with_s else None
    ref, bound = gc.sigmoid_bwd_pad_ref(dy, s if with_s else None, ld)
    flags = torch.cat([torch.zeros(B * TH * TW, dtype=torch.uint8), torch.full((16,), 7, dtype=torch.uint8)]).to(dev)
    out, plain = Out(ref.size, dev), Out(ref.size, dev)
    assert lib.rn_sigmoid_bwd_pad_flags(wg.data_ptr() + 4 * off, sp, out.ptr(), B, H, W, C, ld, stride, None, flags.data_ptr(), st()) == 0
    assert lib.rn_sigmoid_bwd_pad(wg.data_ptr() + 4 * off, sp, plain.ptr(), B, H * W, C, ld, stride, None, st()) == 0
    assert gc.same_bits(out.get(), plain.get())
    bounded("sigmoid_bwd_pad_flags out", out.get(ref.shape), ref, bound)
    f = flags.cpu().numpy()
    assert (f[B * TH * TW:] == 7).all(), "the bytes behind the flags were written"
    assert gc.same_bits(f[:B * TH * TW].reshape(B, TH, TW), gc.flags_ref(H, W, pixels))


@pytest.mark.parametrize("rows,C,ld", gc.COLSUM)
def test_colsum(lib, dev, rows, C, ld):
    g, before = gc.colsum_inputs(rows, C, ld)
    gg = up(g, dev)
    nbytes = lib.rn_colsum_workspace_bytes(rows, C)
    assert nbytes == (rows + gc.CS_ROWS - 1) // gc.CS_ROWS * C * 4
    ws = Out(nbytes, dev, np.uint8)
    out = Out(C, dev)
    assert lib.rn_colsum(gg.data_ptr(), rows, C, ld, out.ptr(), 0, ws.ptr(), st()) == 0
    bounded("colsum", out.get(), *gc.colsum_ref(g, C))
    ws.get()                                                   # (the guard behind the workspace)
    acc = guarded_inout(before, dev)
    assert lib.rn_colsum(gg.data_ptr(), rows, C, ld, acc.ptr(), 1, ws.ptr(), st()) == 0
    bounded("colsum accumulate", acc.get(), *gc.colsum_ref(g, C, before))


@pytest.mark.parametrize("n", gc.RELU_BF16_N)
def test_relu_bf16(lib, dev, n):
    b = gc.relu_bf16_inputs(n)
    src = bf16_dev(b, dev)
    out = Out(n, dev, np.uint16)
    assert lib.rn_relu_bf16(src.data_ptr(), out.ptr(), n, st()) == 0
    want = torch.relu(bf16_dev(b, "cpu")).float().numpy()
    assert gc.same_values(gc.bf16_value(out.get()), want)


@pytest.mark.parametrize("n", gc.ADD_N)
def test_relu_mask(lib, dev, n):
    g, z = gc.synth.normal((n,), 290), gc.signed_zeros(gc.synth.normal((n,), 291), step=5)
    gg = guarded_inout(g, dev)
    assert lib.rn_relu_mask(gg.ptr(), up(z, dev).data_ptr(), n, st()) == 0
    assert gc.same_bits(gg.get(), np.where(z > 0, g, np.float32(0.0)))


@pytest.mark.parametrize("n,per_image", [(k, k) for k in gc.ADD_N] + [(260, 130)])
def test_add_inplace(lib, dev, n, per_image):
    a, b = gc.synth.normal((n,), 292), gc.synth.normal((n,), 293)
    ag = guarded_inout(a, dev)
    assert lib.rn_add_inplace(ag.ptr(), up(b, dev).data_ptr(), n, per_image, None, st()) == 0
    assert gc.same_bits(ag.get(), a + b)


@pytest.mark.parametrize("N,H,W", gc.NHWC4)
def test_nchw_to_nhwc4(lib, dev, N, H, W):
    img = gc.synth.normal((N, 3, H, W), 294)
    want = gc.nhwc4_ref(img)
    out = Out(want.size, dev)
    assert lib.rn_nchw_to_nhwc4(up(img, dev).data_ptr(), out.ptr(), N, H, W, None, st()) == 0
    assert gc.same_bits(out.get(want.shape), want)


# ---------------------------------------------------------------------------------------------- 5. optimizer
@pytest.mark.parametrize("grad_scale,mult", [(1.0, 1.0), (0.25, 4.0)])
def test_clip_adam_past_1024_chunks(lib, dev, grad_scale, mult):
    """1100 one-element parameters, one of 4096 and one of 4097 elements: 1103 chunks, so the norm's final pass wraps its 1024-thread
    loop; three steps, the second one clipped.  Every step is compared with the float64 reference of that step taken from the state the
    kernels themselves left (parameters, moments, and the norm the update kernel read), so each bound is a one-step bound."""
    from retinanet_mi355x.optim import ClipAdam
    sizes, hp = gc.OPT_SIZES, gc.OPT_HP
    offs = np.concatenate([[0], np.cumsum(sizes)])
    pflat = up(np.concatenate(gc.opt_params()), dev)
    gflat = torch.empty_like(pflat)
    params = [torch.nn.Parameter(pflat[offs[i]:offs[i + 1]]) for i in range(len(sizes))]
    opt = ClipAdam(params, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], max_norm=hp["max_norm"], grad_scale=grad_scale)
    assert opt.n_chunks == 1103 == len(gc.opt_chunks(sizes))
    for i, p in enumerate(params):
        p.grad = gflat[offs[i]:offs[i + 1]]
    tag = "clip_adam" if grad_scale == 1.0 else "clip_adam grad_scale"
    for step in range(3):
        grads = gc.opt_grads(step, mult)
        g_in = np.concatenate(grads)
        gflat.copy_(up(g_in, dev))
        p0, m0, v0 = pflat.cpu().numpy(), torch.cat(opt.m).cpu().numpy(), torch.cat(opt.v).cpu().numpy()
        norm = float(opt.step().cpu()[0])
        torch.cuda.synchronize()
        bounded(tag + " norm", norm, *gc.opt_norm_ref(grads, grad_scale))
        assert (norm > hp["max_norm"]) == (step == 1)
        r = gc.opt_step_ref(p0, g_in, m0, v0, np.float32(norm), step + 1, grad_scale)
        bounded(tag + " g", gflat.cpu().numpy(), *r["g"])
        bounded(tag + " m", torch.cat(opt.m).cpu().numpy(), *r["m"])
        bounded(tag + " v", torch.cat(opt.v).cpu().numpy(), *r["v"])
        bounded(tag + " p", pflat.cpu().numpy(), *r["p"])
