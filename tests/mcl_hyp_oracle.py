"""An independent checker of AMCL's pose hypotheses on the KLD filter, written from the definition on top of
the checker of tests/mcl_kld_oracle.py: after a resampling the new set's bins go into a Python dict of integer triples (triple ->
lowest draw), a breadth-first fill over the 26 neighbours labels every component by its lowest draw, the clusters are sorted by
(count descending, label ascending), and each of the seven sums of a hypothesis is the adjacent-pair tree as written,
a[0::2] + a[1::2], over the new set padded with +0.0 to a power of two.  It takes nothing from the library."""
import collections
import math

import numpy as np

import mcl_kld_oracle as ko
import mcl_oracle as mo

HYP_MAX = 8


def empty_hypothesis():
    return dict(label=0, count=0, bins=0, pad=0, weight=0.0, mean=[0.0] * 3, covariance=[0.0] * 9)


def no_hypotheses():
    return dict(fresh=0, n_clusters=0, n_hypotheses=0, n=0, update=0, hyp=[empty_hypothesis() for _ in range(HYP_MAX)])


def tree(a):
    """The adjacent-pair tree over a, its length a power of two."""
    a = np.asarray(a, dtype=np.float64)
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return float(a[0])


def clusters(triples):
    """(label of every draw, {label: number of bins}) of the draws' bin triples."""
    lowest = {}
    for i, t in enumerate(triples):
        lowest.setdefault(t, i)
    label_of, bins = {}, {}
    for t, i in sorted(lowest.items(), key=lambda kv: kv[1]):             # ascending lowest draws: a new component starts at its lowest
        if t in label_of:
            continue
        label_of[t] = i
        bins[i] = 0
        todo = collections.deque([t])
        while todo:
            b = todo.popleft()
            bins[i] += 1
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dz in (-1, 0, 1):                                    # the yaw index does not wrap
                        c = (b[0] + dx, b[1] + dy, b[2] + dz)
                        if c in lowest and c not in label_of:
                            label_of[c] = i
                            todo.append(c)
    return [label_of[t] for t in triples], bins


def hypotheses(x, y, yaw, bin_xy, bin_yaw, update):
    """(the result as a dict, the labels int32 [n]) of the new set x, y, yaw."""
    n = len(x)
    triples = [(ko.bin_index(float(a), bin_xy), ko.bin_index(float(b), bin_xy), ko.bin_index(float(c), bin_yaw)) for a, b, c in zip(x, y, yaw)]
    labels, bins = clusters(triples)
    lab = np.array(labels, dtype=np.int32)
    count = collections.Counter(labels)
    order = sorted(count, key=lambda c: (-count[c], c))
    out = no_hypotheses()
    out.update(fresh=1, n_clusters=len(order), n_hypotheses=min(len(order), HYP_MAX), n=n, update=update)
    P = 1
    while P < n:
        P *= 2
    s, c = mo.sincos_any(yaw)
    terms = (x, y, c, s, x * x, x * y, y * y)
    for q, L in enumerate(order[:HYP_MAX]):
        S = []
        for v in terms:
            a = np.zeros(P)                                                # +0.0 where the draw is not of the hypothesis, and beyond n
            a[:n] = np.where(lab == L, v, 0.0)
            S.append(tree(a))
        W = float(count[L])
        mx, my, mc, ms = S[0] / W, S[1] / W, S[2] / W, S[3] / W
        cov = [0.0] * 9
        cov[0] = S[4] / W - mx * mx
        cov[1] = cov[3] = S[5] / W - mx * my
        cov[4] = S[6] / W - my * my
        ln = math.sqrt(mc * mc + ms * ms)
        cov[8] = (-2.0 * math.log(ln) if ln > 0.0 else math.inf) if ln < 1.0 else 0.0
        out["hyp"][q] = dict(label=L, count=count[L], bins=bins[L], pad=0, weight=W / float(n), mean=[mx, my, math.atan2(S[3], S[2])],
                             covariance=cov)
    return out, lab


class HypFilter(ko.KldFilter):
    """The KLD filter with hypotheses: `hyp` is the result of the last resampling, `labels` its labels."""

    def __init__(self, *a, **kw):
        self.hyp, self.labels = no_hypotheses(), np.zeros(0, dtype=np.int32)
        super().__init__(*a, **kw)

    def init(self, mean, sigma):
        super().init(mean, sigma)
        self.hyp, self.labels = no_hypotheses(), np.zeros(0, dtype=np.int32)

    def upload(self, x, y, yaw, w):
        super().upload(x, y, yaw, w)
        self.hyp, self.labels = no_hypotheses(), np.zeros(0, dtype=np.int32)

    def update(self, odom_delta, points_xyz, **kw):
        res = super().update(odom_delta, points_xyz, **kw)
        if res["resampled"]:                                                # the new set: the ancestors' poses, every weight 1 / n
            self.hyp, self.labels = hypotheses(self.x, self.y, self.yaw, self.kld["bin_xy"], self.kld["bin_yaw"], self.update_count)
        else:
            self.hyp = dict(self.hyp, fresh=0)
        return res
