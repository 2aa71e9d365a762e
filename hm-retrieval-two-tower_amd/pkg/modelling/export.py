"""Export / load of trained towers, the two-tower model and the brute-force
index, and a serving entry point.

The reference saves servable TF SavedModels: the two-tower model and each
tower (two_tower_model.py:176-205, abstract_keras_model.py:120-131) and the
BruteForceIndex, whose call() maps RAW query features to the top-k candidate
id strings (brute_force.py:54-83, 108-114; runner.py:104-105).  Here every
artefact is a directory of data files only — no pickles, nothing executable:

  <name>.pt      tensors (torch.save of a dict of tensors; loaded with
                 torch.load(weights_only=True))
  <name>.json    architecture: features (name, dtype, family, embedding size),
                 tower units, joint embedding size, candidate id column, k
  <name>.npz     string data: each categorical feature's vocabulary, the logQ
                 lookup keys, the index identifiers (numpy.load with
                 allow_pickle=False)

`Retriever` is the serving side: raw feature values in (strings as the
reference's tf.string inputs, floats for numeric features), the query tower
and tt_bruteforce_search on the GPU, candidate identifiers out.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from pkg import dtypes
from pkg.schema.features import Feature, FeatureFamily

__all__ = ["save_tower", "load_tower", "save_two_tower", "load_two_tower", "save_index", "load_index",
           "Retriever"]

FORMAT = "hm-two-tower-amd/1"


# ---- features -------------------------------------------------------------
def _feature_spec(f: Feature) -> dict:
    return {"name": f.name, "dtype": f.dtype.name, "family": f.feature_family.value,
            "embedding_size": f.embedding_size, "max_vocab_size": f.max_vocab_size,
            # sequence features (files written before these fields load as None, "mean")
            "sequence_length": f.sequence_length, "pooling": f.pooling}


def _vocab_arrays(features: Sequence[Feature], prefix: str) -> Dict[str, np.ndarray]:
    out = {}
    for f in features:
        if f.vocab is not None:
            out[f"{prefix}vocab.{f.name}"] = np.asarray(f.vocab, dtype=str)
    return out


def _features_from(specs: List[dict], arrays, prefix: str) -> List[Feature]:
    feats = []
    for s in specs:
        key = f"{prefix}vocab.{s['name']}"
        vocab = [str(v) for v in arrays[key].tolist()] if key in arrays else None
        feats.append(Feature(s["name"], dtypes.as_dtype(s["dtype"]), FeatureFamily(s["family"]),
                             embedding_size=s["embedding_size"], vocab=vocab, max_vocab_size=s["max_vocab_size"],
                             sequence_length=s.get("sequence_length"), pooling=s.get("pooling", "mean")))
    return feats


def _write(path_noext: str, meta: dict, tensors: Dict[str, torch.Tensor], arrays: Dict[str, np.ndarray]) -> None:
    d = os.path.dirname(path_noext)
    if d:
        os.makedirs(d, exist_ok=True)
    torch.save({k: v.detach().cpu().contiguous() for k, v in tensors.items()}, path_noext + ".pt")
    np.savez(path_noext + ".npz", **arrays)
    with open(path_noext + ".json", "w") as fh:
        json.dump(dict(meta, format=FORMAT), fh, indent=1)


def _read(path_noext: str):
    with open(path_noext + ".json") as fh:
        meta = json.load(fh)
    if meta.get("format") != FORMAT:
        raise ValueError(f"{path_noext}.json: unknown format {meta.get('format')!r}")
    tensors = torch.load(path_noext + ".pt", map_location="cpu", weights_only=True)
    with np.load(path_noext + ".npz", allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    return meta, tensors, arrays


def _device(device) -> torch.device:
    from pkg.modelling.device import default_device

    return torch.device(device) if device is not None else default_device()


# ---- towers -----------------------------------------------------------------
def _tower_meta(tower) -> dict:
    return {"kind": "tower", "features": [_feature_spec(f) for f in tower.features],
            "joint_embedding_size": tower.joint_embedding_size, "hidden_units": tower.hidden_units,
            # cosine scoring (files written before these fields load as False, 1.0)
            "normalize": bool(tower.normalize), "output_scale": float(tower.output_scale)}


def save_tower(tower, path_noext: str) -> None:
    """<path>.pt/.json/.npz of one Tower (weights, architecture, vocabularies)."""
    _write(path_noext, _tower_meta(tower), tower.state_dict(), _vocab_arrays(tower.features, ""))


def _build_tower(meta: dict, tensors, arrays, device, prefix: str = ""):
    from pkg.modelling.models.tower import Tower

    feats = _features_from(meta["features"], arrays, "")
    tower = Tower(feats, meta["joint_embedding_size"], meta["hidden_units"], device,
                  normalize=bool(meta.get("normalize", False)), output_scale=float(meta.get("output_scale", 1.0)))
    tower.load_state_dict({k[len(prefix):]: v for k, v in tensors.items() if k.startswith(prefix)})
    return tower


def load_tower(path_noext: str, device=None):
    meta, tensors, arrays = _read(path_noext)
    if meta.get("kind") != "tower":
        raise ValueError(f"{path_noext} is a {meta.get('kind')}, not a tower")
    return _build_tower(meta, tensors, arrays, _device(device))


# ---- two-tower model ----------------------------------------------------------
def save_two_tower(model, path_noext: str) -> None:
    lookup = model.logq_correction.lookup if model.logq_correction is not None else {}
    meta = {"kind": "two_tower", "query_features": [_feature_spec(f) for f in model.query_features],
            "candidate_features": [_feature_spec(f) for f in model.candidate_features],
            "candidate_id_col": model.candidate_id_col,
            "joint_embedding_size": model.query_tower.joint_embedding_size,
            "query_tower_units": model.query_tower.hidden_units,
            "candidate_tower_units": model.candidate_tower.hidden_units,
            "remove_accidental_hits": bool(model.remove_accidental_hits),
            "normalize_embeddings": bool(model.normalize_embeddings), "temperature": model.temperature,
            "num_hard_negatives": model.num_hard_negatives,
            # mixed negative sampling: the setting and its seed (the catalogue itself is not saved)
            "num_sampled_negatives": model.num_sampled_negatives,
            "sampled_negatives_seed": model.sampled_negatives_seed}
    arrays = _vocab_arrays(model.query_features, "query.")
    arrays.update(_vocab_arrays(model.candidate_features, "candidate."))
    arrays["logq.keys"] = np.asarray(list(lookup.keys()), dtype=str)
    arrays["logq.probs"] = np.asarray(list(lookup.values()), dtype=np.float32)
    _write(path_noext, meta, model.state_dict(), arrays)


def load_two_tower(path_noext: str, device=None):
    from pkg.modelling.models.two_tower_model import TwoTowerModel

    meta, tensors, arrays = _read(path_noext)
    if meta.get("kind") != "two_tower":
        raise ValueError(f"{path_noext} is a {meta.get('kind')}, not a two-tower model")
    keys, probs = arrays["logq.keys"], arrays["logq.probs"]
    lookup = {str(k): float(p) for k, p in zip(keys.tolist(), probs.tolist())} or None
    model = TwoTowerModel(_features_from(meta["query_features"], arrays, "query."),
                          _features_from(meta["candidate_features"], arrays, "candidate."),
                          meta["candidate_id_col"], meta["joint_embedding_size"], meta["query_tower_units"],
                          meta["candidate_tower_units"], candidate_prob_lookup=lookup, device=_device(device),
                          remove_accidental_hits=bool(meta.get("remove_accidental_hits", False)),
                          normalize_embeddings=bool(meta.get("normalize_embeddings", False)),
                          temperature=meta.get("temperature"),
                          num_hard_negatives=meta.get("num_hard_negatives"),
                          num_sampled_negatives=meta.get("num_sampled_negatives"),
                          sampled_negatives_seed=int(meta.get("sampled_negatives_seed", 0)))
    model.query_tower.load_state_dict({k[len("query_tower."):]: v for k, v in tensors.items()
                                       if k.startswith("query_tower.")})
    model.candidate_tower.load_state_dict({k[len("candidate_tower."):]: v for k, v in tensors.items()
                                           if k.startswith("candidate_tower.")})
    return model


# ---- brute-force index --------------------------------------------------------
def save_index(index, path_noext: str) -> None:
    """The index's candidates, identifiers and k, plus its query tower, so a
    loaded index answers raw queries on its own (brute_force.py:108-114)."""
    qm = index.query_model
    if not hasattr(qm, "features"):
        raise TypeError("only an index whose query model is a Tower can be exported")
    ident = index._identifiers
    ident = ident.cpu().numpy() if isinstance(ident, torch.Tensor) else np.asarray(ident)
    if ident.dtype.kind == "O":
        ident = ident.astype(str)
    meta = dict(_tower_meta(qm), kind="bruteforce_index", k=index.k)
    tensors = {"candidates": index._candidates}
    tensors.update({f"query_tower.{k}": v for k, v in qm.state_dict().items()})
    arrays = _vocab_arrays(qm.features, "")
    arrays["identifiers"] = ident
    _write(path_noext, meta, tensors, arrays)


def load_index(path_noext: str, device=None):
    from pkg.modelling.indices.brute_force import BruteForceIndex

    meta, tensors, arrays = _read(path_noext)
    if meta.get("kind") != "bruteforce_index":
        raise ValueError(f"{path_noext} is a {meta.get('kind')}, not a brute-force index")
    dev = _device(device)
    tower = _build_tower(meta, tensors, arrays, dev, prefix="query_tower.")
    ident = arrays["identifiers"]
    ids = torch.as_tensor(ident, device=dev) if ident.dtype.kind in "iu" else ident
    return BruteForceIndex(meta["k"], tower, [(ids, tensors["candidates"])], device=dev)


# ---- serving ---------------------------------------------------------------------
class Retriever:
    """Raw query features -> top-k candidate identifiers.

    `Retriever.load(path)` restores an index saved by BruteForceIndex.save
    (with its query tower); `retriever(queries)` takes a dict of raw values
    per query feature — strings (str / bytes / ints, compared as str() like
    the reference's tf.string inputs) for categorical features, numbers for
    numeric ones — and returns the [B, k] identifiers: a numpy string array
    for string identifiers, an int tensor for integer ones.  The StringLookup
    runs in libtt's host hash table, the tower and the exact top-k search on
    the GPU; `scores=True` also returns the fp32 scores."""

    def __init__(self, index):
        self.index = index
        self.tower = index.query_model

    @classmethod
    def load(cls, path_noext: str, device=None) -> "Retriever":
        return cls(load_index(path_noext, device))

    def encode(self, queries: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        return self.tower.input_layer.encode(queries)

    def __call__(self, queries: Dict[str, Any], k: Optional[int] = None, scores: bool = False, exclude=None):
        """exclude: per-query raw identifiers that must not be returned (e.g.
        the articles a customer already has): a list of per-query lists;
        strings for a string-identified index, compared as str() like the
        query features; identifiers the index does not hold are ignored.  The
        result is the exact top-k of the remaining candidates
        (BruteForceIndex.query_with_exclusions)."""
        with torch.no_grad():
            emb = self.tower(self.encode(queries))
            if exclude is None:
                s, idx = self.index.search(emb, k)
            else:
                pos = self.index.exclusion_positions(exclude, int(emb.shape[0]), k)
                s, idx = self.index.search(emb, k, exclusions=pos)
        ids = self.index.lookup_identifiers(idx)
        return (ids, s) if scores else ids
