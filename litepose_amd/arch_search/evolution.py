"""arch_search/evolution.py: one roll-out of regularised evolution over the supernet's search space.

The draws are the reference's, in its order: ``random.randint`` for resolutions and widths, ``random.random`` against
``mutate_prob``, an element-wise ``random.choice`` over the list-valued keys in the crossover, ``np.random.randint`` for
the parents.  ``py_rng`` (a ``random.Random``) and ``np_rng`` (a ``numpy.random.RandomState``) default to the global
generators, which is what the reference draws from; seeded alike, a search replays the reference's population."""
import copy
import random

import numpy as np

from ..models.pose_supermobilenet import ArchManager, _make_divisible

__all__ = ['EvolutionFinder']


class EvolutionFinder(object):
    def __init__(self, cfg, efficiency_predictor, accuracy_predictor, **kwargs):
        self.cfg = cfg
        self.efficiency_predictor = efficiency_predictor
        self.accuracy_predictor = accuracy_predictor
        self.arch_manager = ArchManager(cfg)

        self.mutate_prob = kwargs.get('mutate_prob', 0.1)
        self.population_size = kwargs.get('population_size', 40)
        self.max_time_budget = kwargs.get('max_time_budget', 40)
        self.parent_ratio = kwargs.get('parent_ratio', 0.25)
        self.mutation_ratio = kwargs.get('mutation_ratio', 0.5)
        self.py_rng = kwargs.get('py_rng') or random
        self.np_rng = kwargs.get('np_rng') or np.random
        self.history = []              # one list of (accuracy, sample, efficiency) per generation, in evaluation order

    def set_efficiency_constraint(self, new_constraint):
        self.efficiency_constraint = new_constraint

    # ---- arch_manager.py:5-6,44-69 on the injected generator -----------------------------------
    def _rand(self, c):
        return self.py_rng.randint(0, c - 1)

    def _rand_channel(self, c):
        wm = self.arch_manager.width_mult
        return _make_divisible(c * wm[self._rand(len(wm))], 8)

    def _random_arch(self):
        am = self.arch_manager
        if am.is_search:
            return am.search_arch
        cfg_arch = {}
        cfg_arch['img_size'] = 256 + 64 * self._rand(5)
        cfg_arch['input_channel'] = self._rand_channel(am.input_channel)
        cfg_arch['deconv_setting'] = [self._rand_channel(f) for f in am.deconv_setting]
        cfg_arch['backbone_setting'] = []
        for c, n, s in am.arch_setting:
            cfg_arch['backbone_setting'].append({'num_blocks': n, 'stride': s, 'channel': self._rand_channel(c),
                                                 'block_setting': [[6, 7] for _ in range(n)]})
        return cfg_arch

    def random_sample(self):
        constraint = self.efficiency_constraint
        while True:
            sample = self._random_arch()
            efficiency = self.efficiency_predictor.predict_eff(sample)
            if efficiency <= constraint:
                return sample, efficiency

    def mutate_sample(self, sample):
        constraint = self.efficiency_constraint
        am, rng = self.arch_manager, self.py_rng
        while True:
            cfg_arch = copy.deepcopy(sample)
            if rng.random() < self.mutate_prob:
                cfg_arch['img_size'] = 256 + 64 * self._rand(5)
            if rng.random() < self.mutate_prob:
                cfg_arch['input_channel'] = self._rand_channel(am.input_channel)
            for i in range(len(am.deconv_setting)):
                if rng.random() < self.mutate_prob:
                    cfg_arch['deconv_setting'][i] = self._rand_channel(am.deconv_setting[i])
            for i in range(len(am.arch_setting)):
                if rng.random() < self.mutate_prob:
                    cfg_arch['backbone_setting'][i]['channel'] = self._rand_channel(am.arch_setting[i][0])
            efficiency = self.efficiency_predictor.predict_eff(cfg_arch)
            if efficiency <= constraint:
                return cfg_arch, efficiency

    def crossover_sample(self, sample1, sample2):
        constraint = self.efficiency_constraint
        while True:
            new_sample = copy.deepcopy(sample1)
            for key in new_sample.keys():
                if not isinstance(new_sample[key], list):
                    continue                         # img_size and input_channel stay the first parent's
                for i in range(len(new_sample[key])):
                    new_sample[key][i] = self.py_rng.choice([sample1[key][i], sample2[key][i]])
            efficiency = self.efficiency_predictor.predict_eff(new_sample)
            if efficiency <= constraint:
                return new_sample, efficiency

    def run_evolution_search(self, verbose=False):
        """Run a single roll-out of regularized evolution to a fixed time budget.  Returns the best
        (accuracy, sample, efficiency) among the parents of the generations; ``self.history`` keeps every generation."""
        max_time_budget = self.max_time_budget
        population_size = self.population_size
        mutation_numbers = int(round(self.mutation_ratio * population_size))
        parents_size = int(round(self.parent_ratio * population_size))

        best_valids = [-100]
        population = []                # (validation, sample, efficiency) tuples
        self.history = []
        if verbose:
            print('Generate random population...')
        for k in range(population_size):
            if verbose:
                print(k)
            sample, efficiency = self.random_sample()
            population.append((self.accuracy_predictor.predict_acc(sample), sample, efficiency))
        self.history.append(list(population))

        if verbose:
            print('Start Evolution...')
        for it in range(max_time_budget):
            parents = sorted(population, key=lambda x: x[0])[::-1][:parents_size]
            acc = parents[0][0]
            if verbose:
                print('Iter: {} Acc: {}'.format(it, parents[0][0]))
            if acc > best_valids[0]:
                best_valids = parents[0]

            population = parents
            children = []
            for i in range(mutation_numbers):
                par_sample = population[self.np_rng.randint(parents_size)][1]
                new_sample, efficiency = self.mutate_sample(par_sample)
                children.append((self.accuracy_predictor.predict_acc(new_sample), new_sample, efficiency))
            for i in range(population_size - mutation_numbers):
                par_sample1 = population[self.np_rng.randint(parents_size)][1]
                par_sample2 = population[self.np_rng.randint(parents_size)][1]
                new_sample, efficiency = self.crossover_sample(par_sample1, par_sample2)
                children.append((self.accuracy_predictor.predict_acc(new_sample), new_sample, efficiency))
            population = population + children
            self.history.append(children)

        return best_valids
