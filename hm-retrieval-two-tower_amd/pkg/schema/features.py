from enum import Enum
import logging
from typing import Dict, List, Optional, Sequence

import numpy as np
import pandas as pd

from pkg import dtypes

logger = logging.getLogger(__name__)


class FeatureFamily(Enum):
    """
    The families which features can be part of
    (reference: pkg/schema/features.py:11-18).
    """

    QUERY = "query"
    CANDIDATE = "candidate"


class Feature:
    """
    All of the information for an input feature
    (reference: pkg/schema/features.py:21-127; same arguments and checks).

    Parameters
    ----------
    name: str
        Name of the feature.
    dtype: pkg.dtypes.DType
        ``pkg.dtypes.string`` (categorical, embedded) or ``pkg.dtypes.float32``
        (numeric pass-through).  Strings such as "string" / "tf.string" are
        accepted too.
    feature_family: FeatureFamily
        QUERY or CANDIDATE.
    embedding_size: Optional[int]
        For categorical features, the embedding dimension.
    vocab: Optional[List[str]]
        For categorical features, the values the feature can take.  Unseen
        values map to the OOV row 0.
    max_vocab_size: Optional[int]
        Max size of a vocab built from data (ignored if vocab is given).
    sequence_length: Optional[int]
        L >= 1 makes this a sequence feature: each example carries up to L
        values (its last L are kept), embedded and pooled into one
        embedding_size-wide segment (Keras Embedding + masked pooling).  Only
        for ``pkg.dtypes.string`` with an embedding_size.
    pooling: str
        "mean", "sum" or "sqrtn": how a sequence feature's valid slots are
        combined (TF safe_embedding_lookup_sparse's combiner).

    The id -> row mapping is the reference's StringLookup(num_oov_indices=1)
    (input_layer.py:33-36): vocab[i] -> row i+1, anything else -> row 0.
    """

    VALID_DTYPES = [dtypes.string, dtypes.float32]
    VALID_POOLINGS = ["mean", "sum", "sqrtn"]
    MAX_SEQUENCE_LENGTH = 1024  # tt_gather_bag's slot limit
    PAD_ID = -1                 # the padding id of a sequence feature's slots

    def __init__(
        self,
        name: str,
        dtype,
        feature_family: FeatureFamily,
        embedding_size: Optional[int] = None,
        vocab: Optional[List[str]] = None,
        max_vocab_size: Optional[int] = None,
        sequence_length: Optional[int] = None,
        pooling: str = "mean",
    ):
        self.name = name
        try:
            dtype = dtypes.as_dtype(dtype)
        except TypeError:
            raise TypeError(f"dtype must be one of {self.VALID_DTYPES}, got {dtype}") from None
        if dtype not in self.VALID_DTYPES:
            raise TypeError(f"dtype must be one of {self.VALID_DTYPES}, got {dtype}")
        self.dtype = dtype

        if not isinstance(feature_family, FeatureFamily):
            raise ValueError(
                f"feature_family {feature_family} not valid. "
                f"Must be one of {FeatureFamily._member_names_}"
            )
        self.feature_family = feature_family

        if embedding_size:
            if dtype != dtypes.string:
                raise TypeError(f"Got embedding size, dtype must be tf.string got {dtype}")
        self.embedding_size = embedding_size
        self._lookup: Optional[Dict[str, int]] = None
        self._native = None
        self._init_vocab(vocab)

        if max_vocab_size:
            if not isinstance(max_vocab_size, int):
                raise TypeError(f"max_vocab_size must be an int, got {max_vocab_size}")
        self.max_vocab_size = max_vocab_size

        if sequence_length is not None:
            if isinstance(sequence_length, bool) or not isinstance(sequence_length, int):
                raise TypeError(f"sequence_length must be an int, got {sequence_length}")
            if not 1 <= sequence_length <= self.MAX_SEQUENCE_LENGTH:
                raise ValueError(f"sequence_length must be in 1..{self.MAX_SEQUENCE_LENGTH}, got {sequence_length}")
            if dtype != dtypes.string:
                raise TypeError(f"Got sequence_length, dtype must be tf.string got {dtype}")
            if not embedding_size:
                raise ValueError(f"sequence feature {name} needs an embedding_size")
        if pooling not in self.VALID_POOLINGS:
            raise ValueError(f"pooling {pooling} not valid. Must be one of {self.VALID_POOLINGS}")
        self.sequence_length = sequence_length
        self.pooling = pooling

    @property
    def is_sequence(self) -> bool:
        return self.sequence_length is not None

    def _init_vocab(self, vocab: Optional[List[str]] = None) -> None:
        """Check the dtype and init the vocab (features.py:83-104)."""
        if self.dtype != dtypes.string:
            logger.info(f"Ignoring vocab passed for non-string feature {self.name}")
            self.vocab = None
            self.is_built = True
        else:
            if vocab:
                # The reference stores a set (unordered rows); keep the
                # de-duplicated insertion order so rows are reproducible.
                self.vocab = np.array([str(v) for v in dict.fromkeys(vocab)])
                self.is_built = True
            else:
                self.vocab = None
                self.is_built = False
        self._lookup = None
        self._native = None

    def set_vocab_from_dataframe(self, df: pd.DataFrame) -> None:
        """
        Set the vocabulary from a DataFrame (features.py:106-127):
        value_counts() order, optional head(max_vocab_size), str().
        """
        if self.name not in df.columns:
            raise ValueError(f"Feature name {self.name} not found in df cols {df.columns}")
        col = df[self.name]
        if self.is_sequence:  # count the elements of the per-example sequences
            col = pd.Series([v for seq in col for v in self._elements(seq)], dtype=object)
        v_counts = col.value_counts()
        if self.max_vocab_size:
            vocab = list(v_counts.head(self.max_vocab_size).index)
        else:
            vocab = list(v_counts.index)
        self.vocab = np.array([str(x) for x in vocab])
        self.is_built = True
        self._lookup = None
        self._native = None

    # ---- id encoding (StringLookup) -------------------------------------
    @property
    def num_rows(self) -> int:
        """Embedding table rows: len(vocab) + 1 for the OOV row."""
        if self.vocab is None:
            raise ValueError(f"feature {self.name} has no vocab")
        return len(self.vocab) + 1

    def lookup_table(self) -> Dict[str, int]:
        if self._lookup is None:
            if self.vocab is None:
                raise ValueError(f"feature {self.name} has no vocab")
            self._lookup = {v: i + 1 for i, v in enumerate(self.vocab)}
        return self._lookup

    def encode(self, values: Sequence, num_threads: int = 0) -> np.ndarray:
        """Strings (or anything str()-able) -> int32 rows; OOV -> 0.  Runs in
        libtt's multi-threaded host hash lookup (pkg.schema.vocab), built once
        per vocabulary."""
        if self.vocab is None:
            raise ValueError(f"feature {self.name} has no vocab")
        if self._native is None:
            from pkg.schema.vocab import NativeVocab

            self._native = NativeVocab(self.vocab)
        if self.is_sequence:
            return self._encode_sequences(values, num_threads)
        return self._native.encode(values, num_threads)

    @staticmethod
    def _elements(seq) -> list:
        """One example's values as a list; None / NaN / empty -> []."""
        if seq is None:
            return []
        if isinstance(seq, (list, tuple)):
            return list(seq)
        if isinstance(seq, np.ndarray):
            return seq.reshape(-1).tolist() if seq.ndim else Feature._elements(seq.item())
        if isinstance(seq, (float, np.floating)) and np.isnan(seq):
            return []
        raise TypeError(f"a sequence feature takes a list, tuple or array per example, got {type(seq).__name__}")

    def _encode_sequences(self, values: Sequence, num_threads: int = 0) -> np.ndarray:
        """One sequence per example -> int32 [n, L]: the last L values of each,
        in order, left-aligned and padded with PAD_ID; all elements go through
        one vocabulary lookup."""
        if hasattr(values, "to_numpy") and not isinstance(values, np.ndarray):
            values = values.to_numpy()
        L = self.sequence_length
        if isinstance(values, np.ndarray) and values.ndim == 2 and values.dtype.kind != "O":
            seqs = [row.tolist() for row in values]
        else:
            seqs = [self._elements(seq) for seq in values]
        seqs = [seq[-L:] for seq in seqs]
        out = np.full((len(seqs), L), self.PAD_ID, dtype=np.int32)
        lens = np.fromiter((len(seq) for seq in seqs), dtype=np.int64, count=len(seqs))
        if lens.sum():
            flat = self._native.encode([v for seq in seqs for v in seq], num_threads)
            out[np.arange(L)[None, :] < lens[:, None]] = flat
        return out

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_lookup"] = None
        state["_native"] = None
        return state

    def __setstate__(self, state):
        state.setdefault("_native", None)
        # pickles written before sequence features
        state.setdefault("sequence_length", None)
        state.setdefault("pooling", "mean")
        self.__dict__.update(state)

    def __repr__(self) -> str:
        return (f"Feature({self.name!r}, {self.dtype}, {self.feature_family}, "
                f"embedding_size={self.embedding_size}"
                + (f", sequence_length={self.sequence_length}, pooling={self.pooling!r})" if self.is_sequence
                   else ")"))
