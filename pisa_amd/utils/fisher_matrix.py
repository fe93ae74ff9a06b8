"""Fisher matrix (pisa/utils/fisher_matrix.py): `get_fisher_matrix` at the maker's current state and the
`FisherMatrix` class.

`get_fisher_matrix` takes the fiducial template plus two templates per free parameter.  Where the maker has one
pipeline of the replayable shape whose moving parameters belong to osc.prob3 / aeff.aeff, all 2P + 1 templates
come from one sweep of the events (two for P > 7, `HotPathEngine.eval_many`'s chunks); otherwise each point is one
`get_outputs(return_sum=True)`.  Either way the gradients, the matrix and the nonempty count are one
`pisa_hip_fisher` launch, in the reference's arithmetic and bin order: the matrix equals the reference's
`fmatrix += np.outer(g, g) / sigma` loop bit for bit (sigma being the std dev, as the reference has it).

Deviations from the reference (each has a test):
  * A parameter whose test values are not exactly two distinct values raises ValueError (the reference asserts).
  * A fiducial map without errors raises ValueError (the reference divides by zero).
  * `__add__` orders the parameters as self's, then other's new ones (the reference goes through a `set`, whose
    order depends on the hash seed).
  * `renameParameter` checks the parameter list (the reference indexes it with a bool).
  * `fromPaPAFile` is not ported (it is Python 2 code).
  * `sortByParam` returns the list the reference's `iteritems()` call meant.
  * Pipelines with a variable binning (outputs are lists) raise NotImplementedError.
"""
import copy
import itertools
import operator
import sys

import numpy as np
from scipy.stats import chi2

from pisa_amd.utils.fileio import from_file, to_file

__all__ = ["FisherMatrix", "build_fisher_matrix", "get_fisher_matrix"]

FTYPE = np.float64


def build_fisher_matrix(gradient_hist_flat_d, fiducial_hist, fiducial_params):
    """Fisher matrix of the flat per-parameter gradients and the fiducial MapSet (fisher_matrix.py:41-75), on the
    device: returns (FisherMatrix, nonempty) with the parameters in sorted order and `nonempty` an np.nonzero
    tuple of the fiducial 'total'."""
    import torch

    from pisa_amd import kernels as K

    params = sorted(gradient_hist_flat_d.keys())
    fid = fiducial_hist["total"]
    hist = np.asarray(fid.nominal_values, dtype=FTYPE).ravel()
    n_par, n_bins = len(params), hist.size
    # points: the fiducial, a zero map and the gradients, so that (g - 0) / 1 hands each gradient over unchanged
    pts = np.zeros((n_par + 2, n_bins))
    pts[0] = hist
    for i, p in enumerate(params):
        pts[i + 2] = np.asarray(gradient_hist_flat_d[p], dtype=FTYPE).ravel()
    var = np.zeros_like(pts)
    var[0] = np.asarray(fid.variances, dtype=FTYPE).ravel()
    res = K.fisher(K.to_device(pts), K.to_device(var), [1] * n_par, list(range(2, n_par + 2)), [1.0] * n_par)
    _check_sigma(res)
    fisher = FisherMatrix(matrix=res["matrix"].cpu().numpy(), parameters=params,
                          best_fits=fiducial_params.nominal_values, priors=None)
    torch.cuda.current_stream().synchronize()
    return fisher, np.nonzero(hist)


def _check_sigma(res):
    if res["status"]:
        raise ValueError("the fiducial map has a nonempty bin without error (sigma = 0): the Fisher matrix divides "
                         "by it; evaluate the maker with errors (output_key ('weights', 'errors'))")


def get_fisher_matrix(hypo_maker, test_vals, counter):
    """Fisher matrix at the maker's current state (fisher_matrix.py:78-116).  `test_vals` {name: two values}
    for every free parameter; each is set with `params[name].value = v` in `params.free.names` order and left
    there.  Returns (fisher, gradient_maps {'total': {name: flat gradient}}, fiducial MapSet, nonempty)."""
    hypo_params = hypo_maker.params.free
    names = list(hypo_params.names)
    best_fits = hypo_params.nominal_values
    res = hypo_maker._fisher_templates(names, test_vals)
    counter += 1
    for pname in names:
        counter += len(test_vals[pname])
    _check_sigma(res)
    gradient_maps = {"total": {p: res["grad"][i] for i, p in enumerate(names)}}
    order = sorted(range(len(names)), key=lambda i: names[i])
    params = [names[i] for i in order]
    m = res["matrix"]
    fisher = FisherMatrix(matrix=m[np.ix_(order, order)], parameters=params, best_fits=best_fits, priors=None)
    return fisher, gradient_maps, res["fiducial"], res["nonempty"]


class FisherMatrix:
    """fisher_matrix.py:119-676"""

    def __init__(self, matrix, parameters, best_fits, priors=None, labels=None):
        """matrix: P x P; parameters: names; best_fits: values; priors: Prior objects, numbers or None (None: all
        uniform, sigma = inf); labels: pretty-print labels (default: the names)"""
        self.matrix = np.matrix(matrix)
        self.parameters = list(parameters)
        self.best_fits = list(best_fits)
        if priors is None:
            self.priors = [np.inf for p in self.parameters]
        else:
            self.priors = [self.translatePrior(prior) for prior in priors]
        self.labels = list(labels) if labels is not None else parameters
        self.checkConsistency()
        self.calculateCovariance()

    @classmethod
    def fromFile(cls, filename):
        """a Fisher matrix from a json file written by `saveFile`"""
        return cls(**from_file(filename))

    def __add__(self, other):
        # merge parameter lists: self's, then other's new ones
        new_params = list(self.parameters) + [p for p in other.parameters if p not in self.parameters]
        new_best_fits = []
        new_labels = []
        for param in new_params:
            try:
                value = self.getBestFit(param)
                lbl = self.getLabel(param)
            except IndexError:
                value = other.getBestFit(param)
                lbl = other.getLabel(param)
            new_best_fits.append(value)
            new_labels.append(lbl)
        new_matrix = np.matrix(np.zeros((len(new_params), len(new_params))))
        for (i, j) in itertools.product(range(len(new_params)), range(len(new_params))):
            for summand in [self, other]:
                try:
                    i_sum = summand.getParameterIndex(new_params[i])
                    j_sum = summand.getParameterIndex(new_params[j])
                except IndexError:
                    continue
                new_matrix[i, j] += summand.matrix[i_sum, j_sum]
        new_object = FisherMatrix(matrix=new_matrix, parameters=new_params, best_fits=new_best_fits,
                                  labels=new_labels)
        new_object.calculateCovariance()
        # fill in priors
        for par in new_object.parameters:
            for summand in [self, other]:
                try:
                    prior_dict = summand.getPriorDict()
                except IndexError:
                    continue
                for par, sigma in prior_dict.items():
                    new_object.addPrior(par, sigma)
        return new_object

    def checkConsistency(self):
        """number of parameters matches the matrix, the matrix is symmetric, names are unique, and best_fits,
        labels and priors have one entry per parameter"""
        if not len(self.parameters) == np.shape(self.matrix)[1]:
            raise IndexError("Number of parameters does not match dimension of Fisher matrix! [%i, %i]"
                             % (len(self.parameters), len(self.matrix)))
        if not np.all(self.matrix.T == self.matrix):
            raise ValueError("Fisher matrix not symmetric!")
        if not len(self.parameters) == len(set(self.parameters)):
            raise ValueError("Parameter names not unique! %s" % (np.array2string(np.array(self.parameters))))
        if not len(self.parameters) == len(self.best_fits) == len(self.labels) == len(self.priors):
            raise ValueError("Parameters, best_fits, labels, and priors must all have same length! "
                             "(lengths = %d, %d, %d, %d)" % (len(self.parameters), len(self.best_fits),
                                                             len(self.labels), len(self.priors)))
        return True

    def saveFile(self, filename):
        """write the Fisher matrix to a json file"""
        dict_to_write = {}
        dict_to_write["matrix"] = np.asarray(self.matrix)
        dict_to_write["parameters"] = self.parameters
        dict_to_write["best_fits"] = self.best_fits
        dict_to_write["labels"] = self.labels
        dict_to_write["priors"] = self.priors
        to_file(dict_to_write, filename)

    def getParameterIndex(self, par):
        if par not in self.parameters:
            raise IndexError("%s not found in parameter list %s"
                             % (par, np.array2string(np.array(self.parameters))))
        return self.parameters.index(par)

    def renameParameter(self, fromname, toname):
        idx = self.getParameterIndex(fromname)
        if toname in [p for p in self.parameters if p != fromname]:
            raise ValueError("%s already in parameter list %s"
                             % (toname, np.array2string(np.array(self.parameters))))
        self.parameters[idx] = toname

    def calculateCovariance(self):
        """covariance = inv(F + diag(1 / prior^2))"""
        if np.linalg.det(self.matrix) == 0:
            raise ValueError("Fisher Matrix is singular, cannot be inverted!")
        self.covariance = np.linalg.inv(
            self.matrix + np.diag([1. / self.getPrior(p) ** 2 for p in self.parameters])
        )

    def getBestFit(self, par):
        return self.best_fits[self.getParameterIndex(par)]

    def getLabel(self, par):
        return self.labels[self.getParameterIndex(par)]

    def setLabel(self, par, newlabel):
        self.labels[self.getParameterIndex(par)] = newlabel

    def removeParameter(self, par):
        """remove par from the Fisher matrix and recalculate the covariance"""
        idx = self.getParameterIndex(par)
        self.parameters.pop(idx)
        self.best_fits.pop(idx)
        self.labels.pop(idx)
        self.priors.pop(idx)
        self.matrix = np.delete(np.delete(self.matrix, idx, axis=0), idx, axis=1)
        self.checkConsistency()
        self.calculateCovariance()

    @staticmethod
    def translatePrior(prior):
        """Prior object (gaussian or uniform), number or None -> sigma (np.inf for uniform or None)"""
        if np.isscalar(prior):
            return float(prior)
        if prior is None:
            return np.inf
        if prior.kind == "uniform":
            return np.inf
        elif prior.kind == "gaussian":
            return prior.sigma
        else:
            raise TypeError("Prior object must be of either gaussian or uniform kind; got kind `"
                            + str(prior.kind) + "` instead")

    def setPrior(self, par, sigma):
        idx = self.getParameterIndex(par)
        self.priors[idx] = sigma
        self.calculateCovariance()

    def addPrior(self, par, sigma):
        """add a prior of width sigma to the existing one of par, in quadrature"""
        idx = self.getParameterIndex(par)
        self.priors[idx] = 1. / np.sqrt(1. / self.priors[idx] ** 2 + 1. / sigma ** 2)
        self.calculateCovariance()

    def removeAllPriors(self):
        self.priors = [np.inf for p in self.parameters]
        self.calculateCovariance()

    def getPrior(self, par):
        return self.priors[self.getParameterIndex(par)]

    def getPriorDict(self):
        return dict(zip(self.parameters, self.priors))

    def getCovariance(self, par1, par2):
        idx1, idx2 = self.getParameterIndex(par1), self.getParameterIndex(par2)
        return self.covariance[idx1, idx2]

    def getVariance(self, par):
        return self.getCovariance(par, par)

    def getSigma(self, par):
        """standard deviation of par, marginalised over all other parameters"""
        return np.sqrt(self.getVariance(par))

    def getSigmaNoPriors(self, par):
        """standard deviation of par, marginalised over all other parameters, without the prior on par"""
        idx = self.getParameterIndex(par)
        temp_priors = copy.deepcopy(self.priors)
        temp_priors[idx] = np.inf
        temp_covariance = np.linalg.inv(self.matrix + np.diag([1. / s ** 2 for s in temp_priors]))
        return np.sqrt(temp_covariance[idx, idx])

    def getSigmaStatistical(self, par):
        """standard deviation of par with all other parameters fixed"""
        idx = self.getParameterIndex(par)
        return 1. / np.sqrt(self.matrix[idx, idx])

    def getSigmaSystematic(self, par):
        """standard deviation of par for infinite statistics"""
        return np.sqrt(self.getSigmaNoPriors(par) ** 2 - self.getSigmaStatistical(par) ** 2)

    def getErrorEllipse(self, par1, par2, confLevel=0.6827):
        """(a, b, tan(2 theta)) of the confLevel error ellipse in the par1-par2 plane (arXiv:0906.4123)"""
        sigma1, sigma2 = self.getSigma(par1), self.getSigma(par2)
        cov = self.getCovariance(par1, par2)
        if sigma1 > sigma2:
            a_sq = (sigma1 ** 2 + sigma2 ** 2) / 2. + np.sqrt((sigma1 ** 2 - sigma2 ** 2) ** 2 / 4. + cov ** 2)
            b_sq = (sigma1 ** 2 + sigma2 ** 2) / 2. - np.sqrt((sigma1 ** 2 - sigma2 ** 2) ** 2 / 4. + cov ** 2)
        else:
            a_sq = (sigma2 ** 2 + sigma1 ** 2) / 2. - np.sqrt((sigma2 ** 2 - sigma1 ** 2) ** 2 / 4. + cov ** 2)
            b_sq = (sigma2 ** 2 + sigma1 ** 2) / 2. + np.sqrt((sigma2 ** 2 - sigma1 ** 2) ** 2 / 4. + cov ** 2)
        tan_2_th = 2. * cov / (sigma1 ** 2 - sigma2 ** 2)
        scaling = np.sqrt(chi2.ppf(confLevel, 2))
        return scaling * np.sqrt(a_sq), scaling * np.sqrt(b_sq), tan_2_th

    def getCorrelation(self, par1, par2):
        return self.getCovariance(par1, par2) / (self.getSigma(par1) * self.getSigma(par2))

    def printResults(self, parameters=None, file=None):
        """statistical and systematic errors, priors and best fits of the given (default: all) parameters"""
        pars = parameters if parameters is not None else copy.deepcopy(self.parameters)
        pars.sort()
        if file is not None:
            orig_stdout = sys.stdout
            sys.stdout = open(file, "w")
        try:
            param_width = max([max([len(name) for name in pars]), len("parameters")])
            header = (param_width, "parameter", "best fit", "full", "stat", "syst", "priors")
            print("%*s     %9s     %9s     %9s     %9s     %9s" % header)
            print("-" * (70 + param_width))
            for par in pars:
                result = (param_width, par, self.getBestFit(par), self.getSigma(par),
                          self.getSigmaStatistical(par), self.getSigmaSystematic(par), self.getPrior(par))
                par_str = "%*s    %10.3e     %.3e     %.3e     %.3e     %.3e" % result
                print(par_str.replace("inf", "free"))
        finally:
            if file is not None:
                sys.stdout.close()
                sys.stdout = orig_stdout

    def printResultsSorted(self, par, file=None, latex=False):
        """the same, sorted by the impact on par"""
        if file is not None:
            orig_stdout = sys.stdout
            sys.stdout = open(file, "w")
        try:
            if latex:
                print("\\begin{tabular}{lrrrrrr} \n\\toprule")
                print("Parameter & Impact & Best Fit & Full & Stat. & Syst. & Prior \\\\ \n\\midrule")
            else:
                param_width = max([max([len(name) for name in self.parameters]), len("parameters")])
                header = (param_width, "parameter", "impact [%]", "best fit", "full", "stat", "syst", "priors")
                print("%*s     %10s     %9s     %9s     %9s     %9s     %9s" % header)
                print("-" * (85 + param_width))
            for (p, impact) in self.sortByParam(par):
                if latex:
                    result = (self.getLabel(p), impact, self.getBestFit(p), self.getSigma(p),
                              self.getSigmaStatistical(p), self.getSigmaSystematic(p), self.getPrior(p))
                    par_str = "%s & %.1f & \\num{%.2e} & \\num{%.2e} & \\num{%.2e} & \\num{%.2e} & \\num{%.2e} \\\\" % result
                    par_str = par_str.replace("\\num{inf}", "free")
                else:
                    result = (param_width, p, impact, self.getBestFit(p), self.getSigma(p),
                              self.getSigmaStatistical(p), self.getSigmaSystematic(p), self.getPrior(p))
                    par_str = "%*s          %5.1f    %10.3e     %.3e     %.3e     %.3e     %.3e" % result
                    par_str = par_str.replace("inf", "free")
                print(par_str)
            if latex:
                print("\\bottomrule \n\\end{tabular}")
        finally:
            if file is not None:
                sys.stdout.close()
                sys.stdout = orig_stdout

    def sortByParam(self, par):
        """[(parameter, impact)] with impact = correlation(p, par)^2 * 100, descending (par itself first)"""
        impact = dict([[p, self.getCorrelation(p, par) ** 2 * 100] for p in self.parameters])
        return sorted(impact.items(), key=operator.itemgetter(1), reverse=True)
