"""tests/golden/rd_search_samples.npz: the built sample sets of rd_search_inputs (d) as bit patterns, and what the real reference's
find_best_dictionary / build_left_parts_dictionary answered for each of them (chosen cut and every forced cut 1..16): widths, dictionary size,
dictionary, estimate and the whole sorted list.  Data only; written by tools/make_rd_search_golden.py where the reference is built."""
import os

import numpy as np

import rd_search_inputs as inputs

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rd_search_samples.npz")
CUTS = tuple(range(17))  # 0 = the cut the search chooses


def record(checkers):
    """checkers = {64: double checker, 32: float checker} with rd_state_from_samples -> the arrays of the fixture"""
    out = {}
    for bits, chk in checkers.items():
        fdt, udt = inputs.types(bits)
        sets = inputs.synthetic_sample_sets(bits)
        p = f"f{bits}__"
        out[p + "names"] = np.array(list(sets))
        out[p + "sample_offsets"] = np.concatenate([[0], np.cumsum([a.size for a in sets.values()])]).astype(np.int64)
        out[p + "sample_bits"] = np.concatenate([a.view(udt) for a in sets.values()])
        res = [chk.rd_state_from_samples(a, cut) for a in sets.values() for cut in CUTS]
        out[p + "widths"] = np.array([[r["rbw"], r["lbw"], r["dict_size"]] for r in res], np.uint8).reshape(len(sets), len(CUTS), 3)
        out[p + "dict"] = np.array([r["dict"] for r in res], np.uint16).reshape(len(sets), len(CUTS), 8)
        out[p + "estimate"] = np.array([r["estimate"] for r in res], np.float64).reshape(len(sets), len(CUTS))
        out[p + "sorted_offsets"] = np.concatenate([[0], np.cumsum([r["sorted"].size for r in res])]).astype(np.int64)
        out[p + "sorted"] = np.concatenate([r["sorted"] for r in res]).astype(np.uint16)
    return out


def cases(bits, z=None):
    """{name: (samples, [answer of cut 0 (chosen), 1, .., 16])}, an answer being the dict rd_state_from_samples returns"""
    z = np.load(PATH) if z is None else z
    z = {k: z[k] for k in z.files}  # (an .npz member is decompressed at every access)
    fdt, udt = inputs.types(bits)
    p = f"f{bits}__"
    so, to = z[p + "sample_offsets"], z[p + "sorted_offsets"]
    out = {}
    for i, nm in enumerate(str(x) for x in z[p + "names"]):
        smp = z[p + "sample_bits"][so[i]:so[i + 1]].view(fdt)
        ans = []
        for c in CUTS:
            j = i * len(CUTS) + c
            w = z[p + "widths"][i, c]
            ans.append(dict(rbw=int(w[0]), lbw=int(w[1]), dict_size=int(w[2]), dict=z[p + "dict"][i, c], estimate=float(z[p + "estimate"][i, c]),
                            sorted=z[p + "sorted"][to[j]:to[j + 1]]))
        out[nm] = (smp, ans)
    return out


def same_answer(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("rbw", "lbw", "dict_size", "dict", "estimate", "sorted"))
