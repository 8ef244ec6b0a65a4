"""Greedy association (F:abst/feature/associate, F:alg/feature/associate, F:factory/feature/associate).
  FactoryAssociation.greedy / AssociateDescription   F:factory/feature/associate/FactoryAssociation.java:51-65 ; F:abst/feature/associate/AssociateDescription.java:42-61"""
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .core import Context, IllegalArgumentException, _check, _PinnedPool
from .image import TupleDesc_B, TupleDesc_F64

__all__ = ["AssociateDescription", "AssociateSurfBasic", "AssociatedIndex", "FactoryAssociation", "MatchScoreType", "ScoreAssociateEuclideanSq_F64",
           "ScoreAssociateEuclidean_F64", "ScoreAssociateHamming_B", "WrapAssociateSurfBasic"]


@dataclass
class AssociatedIndex:
    """F:struct/feature/AssociatedIndex.java:30-34"""
    src: int = 0
    dst: int = 0
    fitScore: float = 0.0


class MatchScoreType:
    NORM_ERROR = "NORM_ERROR"


class ScoreAssociateEuclideanSq_F64:
    """F:abst/feature/associate/ScoreAssociateEuclideanSq_F64.java -> DescriptorDistance.euclideanSq"""
    kind, sqrt = "l2", 0

    def getScoreType(self):
        return MatchScoreType.NORM_ERROR


class ScoreAssociateEuclidean_F64:
    kind, sqrt = "l2", 1

    def getScoreType(self):
        return MatchScoreType.NORM_ERROR


class ScoreAssociateHamming_B:
    kind, sqrt = "hamming", 0

    def getScoreType(self):
        return MatchScoreType.NORM_ERROR


class AssociateDescription:
    """WrapAssociateGreedy (F:abst/feature/associate/WrapAssociateGreedy.java:73-123) over AssociateGreedy on the GPU."""

    def __init__(self, score, maxError, backwardsValidation, ctx=None):
        self.ctx = ctx or Context.default()
        self.score = score
        self.maxFitError = float(maxError)
        self.backwardsValidation = bool(backwardsValidation)
        self.listSrc = None
        self.listDst = None
        self._matches = []
        self._unassocSrc = []
        self._pairs = np.zeros(0, dtype=np.int32)
        self._fit = np.zeros(0)
        self._nd = 0

    def setSource(self, listSrc):
        self.listSrc = listSrc

    def setDestination(self, listDst):
        self.listDst = listDst

    @staticmethod
    def _pack(lst, kind):
        if isinstance(lst, np.ndarray):
            return np.ascontiguousarray(lst, dtype=np.float64 if kind == "l2" else np.int32)
        if len(lst) == 0:
            return np.zeros((0, 1), dtype=np.float64 if kind == "l2" else np.int32)
        if kind == "l2":
            return np.ascontiguousarray(np.stack([np.asarray(d.value, dtype=np.float64) for d in lst]))
        return np.ascontiguousarray(np.stack([np.asarray(d.data, dtype=np.int32) for d in lst]))

    def associate(self):
        if self.listSrc is None:
            raise IllegalArgumentException("source features not specified")
        if self.listDst is None:
            raise IllegalArgumentException("destination features not specified")
        kind = self.score.kind
        src = self._pack(self.listSrc, kind)
        dst = self._pack(self.listDst, kind)
        ns, nd = len(src), len(dst)
        length = src.shape[1] if ns else (dst.shape[1] if nd else 1)
        if ns and nd and src.shape[1] != dst.shape[1]:
            raise IllegalArgumentException("descriptor lengths differ")
        pairs, fit = _PinnedPool.arrays(self.ctx, [((ns,), np.int32), ((ns,), np.float64)])
        pairs[:] = -1
        fit[:] = self.maxFitError
        L = _lib.load()
        if ns:
            if kind == "l2":
                _check(self.ctx, L.bhip_assoc_l2_f64(self.ctx._h, src.ctypes.data_as(_lib._dp), ns, dst.ctypes.data_as(_lib._dp), nd, length,
                                                     self.maxFitError, int(self.backwardsValidation), self.score.sqrt,
                                                     pairs.ctypes.data_as(_lib._ip), fit.ctypes.data_as(_lib._dp)))
            else:
                _check(self.ctx, L.bhip_assoc_hamming(self.ctx._h, src.ctypes.data_as(_lib._i32p), ns, dst.ctypes.data_as(_lib._i32p), nd, length,
                                                      self.maxFitError, int(self.backwardsValidation), pairs.ctypes.data_as(_lib._ip),
                                                      fit.ctypes.data_as(_lib._dp)))
        self._pairs, self._fit, self._nd = pairs, fit, nd
        self._matches = None      # the object lists are built when they are asked for (getMatches / getUnassociatedSource)
        self._unassocSrc = None

    @property
    def matches(self):
        if self._matches is None:
            idx = np.nonzero(self._pairs >= 0)[0]
            self._matches = [AssociatedIndex(i, d, f) for i, d, f in zip(idx.tolist(), self._pairs[idx].tolist(), self._fit[idx].tolist())]
        return self._matches

    @property
    def unassocSrc(self):
        if self._unassocSrc is None:
            self._unassocSrc = np.nonzero(self._pairs < 0)[0].tolist()
        return self._unassocSrc

    def getPairs(self):
        return self._pairs

    def getFitQuality(self):
        return self._fit

    def getMatches(self):
        return self.matches

    def getUnassociatedSource(self):
        return self.unassocSrc

    def getUnassociatedDestination(self):
        # FindUnassociated.checkDestination (F:alg/feature/associate/FindUnassociated.java:56-72)
        matched = np.zeros(self._nd, dtype=bool)
        for m in self.matches:
            matched[m.dst] = True
        return [i for i in range(self._nd) if not matched[i]]

    def setMaxScoreThreshold(self, score):
        self.maxFitError = float(score)

    def getScoreType(self):
        return self.score.getScoreType()

    def uniqueSource(self):
        return True

    def uniqueDestination(self):
        return self.backwardsValidation


class AssociateSurfBasic:
    """F:alg/feature/associate/AssociateSurfBasic.java:36-170: SURF features are split by the sign of the Laplacian (BrightFeature.white)
    and each sign is associated on its own -- features of different sign are never matched and each contraction is a quarter of the size."""

    def __init__(self, assoc):
        self.assoc = assoc
        self._src = ([], [])   # (positive, negative) lists of (index, feature)
        self._dst = ([], [])
        self.matches = []
        self.unassociatedSrc = []

    @staticmethod
    def _sort(features):
        pos, neg = [], []
        for i, f in enumerate(features):
            (pos if f.white else neg).append((i, f))
        return pos, neg

    def setSrc(self, src):
        self._src = self._sort(src)

    def setDst(self, dst):
        self._dst = self._sort(dst)

    def swapLists(self):
        self._src, self._dst = self._dst, self._src

    def associate(self):
        self.matches = []
        self.unassociatedSrc = []
        if not (self._src[0] or self._src[1]) or not (self._dst[0] or self._dst[1]):
            return
        for sign in (0, 1):   # positive, then negative
            s, d = self._src[sign], self._dst[sign]
            self.assoc.setSource([f for _, f in s])
            self.assoc.setDestination([f for _, f in d])
            self.assoc.associate()
            for a in self.assoc.getMatches():
                self.matches.append(AssociatedIndex(s[a.src][0], d[a.dst][0], a.fitScore))
            self.unassociatedSrc.extend(s[i][0] for i in self.assoc.getUnassociatedSource())

    def getMatches(self):
        return self.matches

    def totalDestination(self):
        return len(self._dst[0]) + len(self._dst[1])

    def getUnassociatedSrc(self):
        return self.unassociatedSrc

    def getAssoc(self):
        return self.assoc


class WrapAssociateSurfBasic:
    """F:abst/feature/associate/WrapAssociateSurfBasic.java:33-101"""

    def __init__(self, alg):
        self.alg = alg

    def setSource(self, listSrc):
        self.alg.setSrc(listSrc)

    def setDestination(self, listDst):
        self.alg.setDst(listDst)

    def associate(self):
        self.alg.associate()

    def getMatches(self):
        return self.alg.getMatches()

    def getUnassociatedSource(self):
        return self.alg.getUnassociatedSrc()

    def getUnassociatedDestination(self):
        # FindUnassociated.checkDestination (F:alg/feature/associate/FindUnassociated.java:56-72)
        n = self.alg.totalDestination()
        matched = np.zeros(n, dtype=bool)
        for m in self.alg.getMatches():
            matched[m.dst] = True
        return [i for i in range(n) if not matched[i]]

    def setMaxScoreThreshold(self, score):
        self.alg.getAssoc().setMaxScoreThreshold(score)

    def getScoreType(self):
        return self.alg.getAssoc().getScoreType()

    def uniqueSource(self):
        return self.alg.getAssoc().uniqueSource()

    def uniqueDestination(self):
        return self.alg.getAssoc().uniqueDestination()


class FactoryAssociation:
    @staticmethod
    def greedy(score, maxError, backwardsValidation, ctx=None):
        return AssociateDescription(score, maxError, backwardsValidation, ctx)

    @staticmethod
    def defaultScore(tupleType):
        """F:factory/feature/associate/FactoryAssociation.java:141-156"""
        if issubclass(tupleType, TupleDesc_F64):
            return ScoreAssociateEuclideanSq_F64()
        if tupleType is TupleDesc_B:
            return ScoreAssociateHamming_B()
        raise IllegalArgumentException("Unknown tuple type: %s" % tupleType)
