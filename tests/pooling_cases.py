"""Golden cases with MaskedAveragePooling sequence fields (sequence.py:21-29), shared by tests/golden/make_golden_pooling.py
(reference side) and tests/test_avg_pooling.py / tests/test_gpu_avg_pooling.py.

Each case is an existing golden_cases.CASES entry with some sequence fields switched to ``MaskedAveragePooling`` (and, for the
d = 64 geometry, two of its categorical fields turned into bags); the fixtures are ``tests/golden/<name>.npz``.  The tests put
these cases into ``golden_cases.CASES`` (monkeypatch) so that model_cases.check_* run on them unchanged.
"""
import golden_cases as gc


def _avg(name, vocab, max_len=3):
    f = gc._seq(name, vocab, max_len)
    f["encoder"] = "MaskedAveragePooling"
    return f


def _derive(base, name, fields, **over):
    case = dict(gc.case_by_name(base), name=name, fields=fields)
    case.update(over)
    return case


_TINY = [gc._cat("a", 7), gc._cat("b", 5), _avg("c", 6), gc._cat("e", 9, padding_idx=8)]
_KKBOX = [_avg("genre_ids", 17) if f["name"] == "genre_ids" else f for f in gc.case_by_name("kkbox_shape")["fields"]]
# d = 64 (the rows64 gather kernel): the north-star fields with two bags, one averaged and one summed
_NORTHSTAR = gc.case_by_name("northstar_shape")["fields"][:18] + [_avg("s18", 37, 4), gc._seq("s19", 37, 4)]

CASES = [
    # BN, wide, embedding L2, bags of 0..max_len real ids
    _derive("tiny_seq_bn", "avgpool_tiny_seq_bn", _TINY),
    # the shipped KKBox geometry (13 fields / 17 columns, d = 40: the vectorised gather): genre_ids averaged, artist_name summed
    _derive("kkbox_shape", "avgpool_kkbox_shape", _KKBOX, embedding_dim=40),
    _derive("northstar_shape", "avgpool_northstar_shape", _NORTHSTAR),
    _derive("m0_tiny_seq", "avgpool_m0_tiny_seq", _TINY),
    _derive("m1_tiny_seq", "avgpool_m1_tiny_seq", _TINY),
    _derive("m3_tiny_seq", "avgpool_m3_tiny_seq", _TINY),
]

NAMES = [c["name"] for c in CASES]


def register(monkeypatch):
    """make the cases visible to golden_cases.case_by_name (and so to model_cases.check_*)"""
    monkeypatch.setattr(gc, "CASES", gc.CASES + [c for c in CASES if c["name"] not in {x["name"] for x in gc.CASES}])


# ----------------------------------------------------------------------------- kernel-level statement (fp64 numpy)
class Field:
    def __init__(self, col, ncols, vocab, padding_idx=None, pooling="sum"):
        self.col, self.ncols, self.vocab, self.padding_idx, self.pooling = col, ncols, vocab, padding_idx, pooling


def kernel_problem(d, B, T, seed=0, fields=None, grads=True):
    """fields (categorical, averaged / summed bags), tables holding exact 0.0 and -0.0 elements in non-padding rows and all-zero
    padding rows, ids that hit padding_idx and whole bags of padding, a label table, label ids and incoming gradients"""
    import numpy as np
    rs = np.random.RandomState(seed)
    if fields is None:
        fields = [Field(0, 1, 7), Field(1, 3, 6, padding_idx=5, pooling="average"), Field(4, 2, 8, padding_idx=7),
                  Field(6, 4, 9, padding_idx=8, pooling="average"), Field(10, 1, 5, padding_idx=4)]
    L = max(f.col + f.ncols for f in fields)
    tables = []
    for f in fields:
        t = rs.standard_normal((f.vocab, d)).astype(np.float32)
        u = rs.rand(f.vocab, d)
        t[u < 0.15] = 0.0
        t[(u >= 0.15) & (u < 0.3)] = -0.0
        if f.padding_idx is not None:
            t[f.padding_idx] = 0.0
        tables.append(t)
    idx = np.zeros((B, T, L), dtype=np.int32)
    for f in fields:
        ids = rs.randint(0, f.vocab, size=(B, T, f.ncols))
        if f.padding_idx is not None and f.ncols > 1:
            ids[rs.rand(B, T) < 0.2] = f.padding_idx                        # all-padding bags
        idx[..., f.col:f.col + f.ncols] = ids
    labels = rs.randint(0, 2, size=(B, T)).astype(np.int32)
    labels[:, 0] = 2
    label_table = rs.standard_normal((3, d)).astype(np.float32)
    if not grads:
        return fields, tables, idx, labels, label_table, None, None
    dgrid = rs.standard_normal((B, T, len(fields) + 1, d)).astype(np.float32)
    dflat = rs.standard_normal((B, len(fields) * d)).astype(np.float32)
    return fields, tables, idx, labels, label_table, dgrid, dflat


def _bag(f, table, ids):
    """-> (fp64 sum, fp32 denominator or None) of one bag, per element"""
    import numpy as np
    rows = table[ids.astype(np.int64)]                                      # [n, d] float32
    s = rows.astype(np.float64).sum(0)
    if f.pooling != "average":
        return s, None
    cnt = (rows != 0).sum(0)
    return s, (cnt.astype(np.float32) + np.float32(1e-16))


def reference_grid(fields, tables, idx, labels, label_table, rows=None):
    """fp64 statement of the forward grid [B][T][S][d] (rows: optional list of (b, t) to evaluate; the others stay nan)"""
    import numpy as np
    B, T, _ = idx.shape
    d = label_table.shape[1]
    out = np.full((B, T, len(fields) + 1, d), np.nan)
    for b, t in (rows if rows is not None else [(b, t) for b in range(B) for t in range(T)]):
        out[b, t, 0] = label_table[labels[b, t]]
        for i, f in enumerate(fields):
            s, den = _bag(f, tables[i], idx[b, t, f.col:f.col + f.ncols])
            out[b, t, 1 + i] = s if den is None else s / den.astype(np.float64)
    return out


def reference_table_grads(fields, tables, idx, dgrid, dflat):
    """fp64 statement of the table gradients and the sum of |terms| of every element (for an accumulation-order tolerance)"""
    import numpy as np
    B, T, _ = idx.shape
    d = tables[0].shape[1]
    grads = [np.zeros(t.shape) for t in tables]
    mags = [np.zeros(t.shape) for t in tables]
    for b in range(B):
        for t in range(T):
            for i, f in enumerate(fields):
                ids = idx[b, t, f.col:f.col + f.ncols]
                _, den = _bag(f, tables[i], ids)
                terms = [dgrid[b, t, 1 + i].astype(np.float64)]
                if t == 0 and dflat is not None:
                    terms.append(dflat[b, i * d:(i + 1) * d].astype(np.float64))
                if den is not None:                 # divided each, then added (fp32 division, as the kernel and torch do)
                    terms = [(term.astype(np.float32) / den).astype(np.float64) for term in terms]
                for j in ids:
                    if j == f.padding_idx:
                        continue
                    for term in terms:
                        grads[i][j] += term
                        mags[i][j] += np.abs(term)
    return grads, mags


def check_pool_kernels(lib, dev, d, B=3, T=4, seed=0):
    """forward of every gather variant the geometry reaches and the averaged backward (scale pass + atomic table stage) against
    the fp64 statement"""
    import numpy as np
    import torch
    from rat_amd import ops
    fields, tables, idx, labels, label_table, dgrid, dflat = kernel_problem(d, B, T, seed)
    F, L = len(fields), idx.shape[2]
    tabs = [torch.from_numpy(t).to(dev) for t in tables]
    ftab = ops.field_table(fields, tabs, dev)
    modes = ops.pool_modes(fields, dev)
    idx_d, labels_d = torch.from_numpy(idx).to(dev), torch.from_numpy(labels).to(dev)
    grid = ops.gather_fwd(idx_d, labels_d, ftab, F, torch.from_numpy(label_table).to(dev), B, T, L, d, modes=modes, lib=lib)
    want = reference_grid(fields, tables, idx, labels, label_table)
    got = grid.cpu().double().numpy()
    scale = np.abs(want).max()
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-6 * scale)
    # sum-only entry point on the same problem: every averaged field's row differs, every other row is bit-identical
    plain = ops.gather_fwd(idx_d, labels_d, ftab, F, torch.from_numpy(label_table).to(dev), B, T, L, d, lib=lib).cpu()
    for i, f in enumerate(fields):
        if f.pooling == "sum":
            assert torch.equal(plain[:, :, 1 + i], grid.cpu()[:, :, 1 + i])
    # backward
    avg = torch.tensor([i for i, f in enumerate(fields) if f.pooling == "average"], dtype=torch.int32, device=dev)
    dg, df = torch.from_numpy(dgrid.copy()).to(dev), torch.from_numpy(dflat.copy()).to(dev)      # scaled in place
    ops.pool_scale_bwd(dg, df, idx_d, ftab, avg, F, B, T, L, d, lib=lib)
    gtabs = [torch.zeros_like(t) for t in tabs]
    gftab = ops.field_table(fields, gtabs, dev)
    ops.gather_bwd(dg, df, idx_d, labels_d, gftab, F, None, B, T, L, d, lib=lib)
    wg, mags = reference_table_grads(fields, tables, idx, dgrid, dflat)
    for i in range(F):
        g = gtabs[i].cpu().double().numpy()
        assert np.all(np.abs(g - wg[i]) <= 1e-5 * mags[i] + 1e-30), (i, float(np.abs(g - wg[i]).max()))
    assert max(float(np.abs(w).max()) for w in wg) > 1e12, "no element with a zero count: the 1e16 path went untested"


def check_pool_gather_large(lib, dev, B=4096, T=11, nfields=20, d=64, rows=512, seed=3):
    """a grid above 160 MB (B 4096, T 11, S 21, d 64: 242 MB): the rows64 gather's non-temporal form, checked on sampled rows"""
    import numpy as np
    import torch
    from rat_amd import ops
    fields, col = [], 0
    for i in range(nfields):
        kind = i % 4                                          # categorical, averaged bag of 3, summed bag of 2, averaged bag of 5
        ncols, pooling = [(1, "sum"), (3, "average"), (2, "sum"), (5, "average")][kind]
        vocab = 500 + 37 * i
        fields.append(Field(col, ncols, vocab, padding_idx=vocab - 1 if ncols > 1 else None, pooling=pooling))
        col += ncols
    fields, tables, idx, labels, label_table, _, _ = kernel_problem(d, B, T, seed, fields=fields, grads=False)
    F, L = len(fields), idx.shape[2]
    assert B * T * (F + 1) * d * 4 > 160 << 20
    tabs = [torch.from_numpy(t).to(dev) for t in tables]
    ftab = ops.field_table(fields, tabs, dev)
    grid = ops.gather_fwd(torch.from_numpy(idx).to(dev), torch.from_numpy(labels).to(dev), ftab, F,
                          torch.from_numpy(label_table).to(dev), B, T, L, d, modes=ops.pool_modes(fields, dev), lib=lib)
    rs = np.random.RandomState(seed + 1)
    pick = sorted({(int(b), int(t)) for b, t in zip(rs.randint(0, B, rows), rs.randint(0, T, rows))} | {(B - 1, T - 1), (0, 0)})
    want = reference_grid(fields, tables, idx, labels, label_table, rows=pick)
    bi = torch.tensor([b for b, _ in pick], device=dev)
    ti = torch.tensor([t for _, t in pick], device=dev)
    got = grid[bi, ti].cpu().double().numpy()
    w = np.stack([want[b, t] for b, t in pick])
    np.testing.assert_allclose(got, w, rtol=2e-6, atol=1e-6 * np.abs(w).max())
