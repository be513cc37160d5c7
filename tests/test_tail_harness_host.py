"""tests/tail_harness.py's comparer held to its own statement, on the CPU: outputs built from the float64 restatement
(rounded to float32, NaN / -7 where no processed row owns an entry, the workspace counts as expected) pass
against_reference for every entry; one compared element moved from the reference by twice its bar (bars()) fails and
names its output, moved by half its bar passes; and each structural fault - an entry that no row owns written, a sample
count, vr_samples, a workgroup count or n_valid off by one, a non-zero behind a stop, a term of the multi entry that is
not named and not +0 - fails and names itself.  On the crafted batch (27 rays) and on its first 9 rows (the second
workgroup with one ray)."""
import numpy as np
import pytest

import tail_harness as H

CASES = [("default", 0), ("masked", 0), ("sem", 0), ("nrm", 0), ("dep", 0), ("multi", 1), ("multi", 2), ("multi", 4), ("multi", 7)]


def setup(entry, mask, n_rays, name="crafted"):
    """-> (x, cfg, ref, noise) of a case"""
    if entry == "multi":
        tg = H.multi_targets(name, 7)
    else:
        tg = dict(labels=H.labels_for(name, 7), normals=H.make_normals(name), depths=H.make_depths(name))
    cfg = dict(n_rays=n_rays, **({"mask": mask, "scene_scale": 0.5} if entry == "multi" else {}))
    if entry == "masked":
        cfg["size_delta"] = 6e-2
    ref, noise = H.reference(entry, name, {k: tg[k] for k in H.ENTRIES[entry]["inputs"] if k in tg}, **cfg)
    return H.batch(name, wide=True), cfg, ref, noise


def baseline(entry, x, cfg, ref):
    """what a faultless launch hands back, as run_entry's `got`: the restatement rounded to float32 (kept in float64, so
    that an element can be moved by an exact multiple of its bar)"""
    e, mask, n_rows = H.ENTRIES[entry], cfg.get("mask", 0), len(x["rays_a"][:cfg.get("n_rays")])
    keys = list(H.PER_RAY) + ["ws", "d_sig", "d_rgb", "terms"] + [k for k in e["outputs"] if k != "workspace" and H.named(entry, k, cfg)]
    got = {k: ref[k].astype(np.float32).astype(np.float64) for k in keys}
    own = np.zeros(x["n_rays"], bool)
    own[x["rays_a"][:cfg.get("n_rays"), 0]] = True
    got["total"], got["vr"] = np.where(own, ref["total"], -7), ref["vr"].copy()
    blocks = (n_rows + 7) // 8
    fit = lambda: ref["fit"].astype(np.float32).astype(np.float64)
    if entry == "sem":
        got["n_valid"] = np.array([ref["n_valid"]] + [0] * 7, np.int32)
    if entry == "nrm":
        got["done"] = np.array([blocks], np.int64)
    if entry == "dep":
        got.update(fit=fit(), n_valid=ref["n_valid"], done=np.array([blocks, blocks], np.int64))
    if entry == "multi":
        S, Nm, D = H.SEM, H.NRM, H.DEP
        got["counts"] = np.array([blocks if mask & S else 0, blocks if mask in (Nm, Nm | D) else 0, blocks if mask & D else 0,
                                  blocks if mask == D else 0], np.int64)
        got["n_valid_labels"] = ref.get("n_valid_labels", 0)
        got["n_valid_depths"] = ref.get("n_valid_depths", 0)
        got["fit"] = fit() if mask & D else np.zeros(2)
    return got


def verdict(entry, got, ref, noise, x, cfg):
    """the comparer's misses, one per line ('' when it passes)"""
    try:
        H.against_reference(entry, "case", got, ref, noise, x, cfg)
    except AssertionError as err:
        return str(err)
    return ""


def movable(got, ref, x, cfg, key, bar):
    """flat indices of the elements of got[key] that are held to a bar above 0 and to nothing else: not the samples that
    must be exactly 0 (behind a stop, without weight or target), not the ray without samples (the background, exactly)"""
    if key in ("terms", "fit"):
        return np.nonzero(bar > 0)[0]
    rows = x["rays_a"][:cfg.get("n_rays")]
    if key in H.PER_SAMPLE:
        sel = H.R.owned(x, cfg.get("n_rays"))[0] >= 0
    else:
        sel = np.zeros(x["n_rays"], bool)
        sel[rows[rows[:, 2] > 0, 0]] = True
    sel = np.broadcast_to(sel.reshape(sel.shape + (1,) * (got[key].ndim - 1)), got[key].shape)
    return np.nonzero((sel & (np.nan_to_num(ref[key]) != 0) & (bar > 0)).ravel())[0]


def moved(got, ref, key, at, by):
    out = dict(got, **{key: got[key].copy()})
    out[key].ravel()[at] = np.ravel(ref[key])[at] + by
    return out


def structural(entry, got, ref, x, cfg):
    """{fault: (got with that fault, what the comparer must say)} for the faults the entry can have"""
    e, mask, n_rays = H.ENTRIES[entry], cfg.get("mask", 0), cfg.get("n_rays")
    rows = x["rays_a"][:n_rays]
    row_of, k_of = H.R.owned(x, n_rays)
    out = {}

    def put(fault, key, at, value, says):
        g = dict(got, **{key: value})
        if isinstance(got[key], np.ndarray):
            g[key] = got[key].copy()
            g[key].ravel()[at] = value
        out[fault] = (g, says)
    put("unowned", "ws", np.nonzero(row_of < 0)[0][0], 0.0, "ws: entries that no processed row owns were written")
    if n_rays is not None:
        ray = np.setdiff1d(np.arange(x["n_rays"]), rows[:, 0])[0]
        put("unowned ray", "opacity", ray, 0.0, "opacity: entries that no processed row owns were written")
        put("unowned count", "total", ray, 0, "total_samples: entries that no processed row owns were written")
    put("total", "total", rows[3, 0], got["total"][rows[3, 0]] + 1, "total_samples: ray")
    put("vr", "vr", 0, got["vr"][0] + 1, "vr_samples:")
    for key in ("done", "counts"):
        if key in got:
            put("counts", key, np.nonzero(got[key])[0][-1], got[key].max() + 1, "workspace:")
    for _, key, _, bit in e.get("n_valid", ()):
        if entry != "multi" or mask & bit:
            put("n_valid" + ("" if entry != "multi" else f" {bit}"), key, 0, np.ravel(got[key])[0] + 1, "n_valid")
    stop = ref["stops"][np.maximum(row_of, 0)]
    behind = np.nonzero((row_of >= 0) & (stop >= 0) & (k_of > stop))[0]
    for key in [k for k in H.PER_SAMPLE if k in got]:
        put(f"behind a stop {key}", key, behind[-1] * (got[key].size // len(got[key])), 1e-30, f"{key}: not exactly 0 behind a stop")
    for slot, bit in H.TERM_BITS if entry == "multi" else ():
        if not mask & bit:
            put(f"unnamed term {slot}", "terms", slot, -0.0, "for a term that is not named")
    return out


@pytest.mark.parametrize("n_rays", [None, 9])
@pytest.mark.parametrize("entry,mask", CASES)
def test_comparer_passes_the_restatement_and_catches_every_fault(entry, mask, n_rays):
    x, cfg, ref, noise = setup(entry, mask, n_rays)
    got = baseline(entry, x, cfg, ref)
    assert verdict(entry, got, ref, noise, x, cfg) == ""                       # (a)
    bar = H.bars(entry, ref, noise, len(x["rays_a"][:n_rays]), cfg)
    assert set(bar) >= {"opacity", "ws", "Ro", "d_sig", "d_rgb", "terms"} | ({"fit"} if "fit" in ref else set())
    for key, b in bar.items():                                                  # (b)
        at = movable(got, ref, x, cfg, key, b)
        assert len(at) or entry == "multi" and key == "terms", key          # (a term that is not named: +0, a bar of 0)
        for i in at if key in ("terms", "fit") else at[[len(at) // 2]]:
            name = {"terms": f"terms[{i}]:", "fit": f"fit {'ab'[i % 2]}:"}.get(key, f"{key}:")
            miss = verdict(entry, moved(got, ref, key, i, 2 * np.ravel(b)[i]), ref, noise, x, cfg).splitlines()
            assert len(miss) == 2 and miss[1].strip().startswith(name), (key, i, miss)
            assert verdict(entry, moved(got, ref, key, i, 0.5 * np.ravel(b)[i]), ref, noise, x, cfg) == "", (key, i)
    faults = structural(entry, got, ref, x, cfg)                               # (c)
    want = {"unowned", "total", "vr", "behind a stop ws", "behind a stop d_sig", "behind a stop d_rgb"}
    want |= {"counts"} if entry in ("nrm", "dep", "multi") else set()
    want |= {"n_valid"} if entry in ("sem", "dep") else set()
    want |= {"n_valid 1", "behind a stop d_sem"} if mask & H.SEM else set()
    want |= {"n_valid 4"} if mask & H.DEP else set()
    want |= {f"unnamed term {slot}" for slot, bit in H.TERM_BITS if entry == "multi" and not mask & bit}
    assert want <= set(faults), want - set(faults)
    for fault, (bad, says) in faults.items():
        miss = verdict(entry, bad, ref, noise, x, cfg)
        assert says in miss, (fault, miss)
