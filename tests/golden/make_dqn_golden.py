"""Generates tests/golden/dqn_known_answers.json: one 2-row, 3-action dueling
double-Q step whose answers are derived by hand from dqn.py:50-71 and
q_net.py:41-65 (nothing here runs a network).  Run:
    python tests/golden/make_dqn_golden.py

D = 2, one hidden layer of 2 units per stream whose first layers are the
identity (observations are positive, so h = obs), gamma = 0.5, B = 2.
  online : adv = WA h, WA = [[1,0],[0,1],[1,1]];  val = 0.5 (h0 + h1) + 0.25
  target : adv = WA' h, WA' = [[0,1],[1,0],[0.5,0.25]] ; val = 0.25 (h0 + h1) + 0.5
Row 0 (terminal, |td| > 1): s = (1, 2), a = 2, r = -2, d = 1, w = 0.5
  adv = (1, 2, 3), mean 2, val 1.75 -> q = (0.75, 1.75, 2.75); y = r = -2;
  td = 4.75; l = 4.75 - 0.5 = 4.25; g = 0.5 * 1 / 2 = 0.25
Row 1 (|td| < 1, double-Q): s = (2, 1), a = 0, r = 0.5, d = 0, s' = (1, 3), w = 1
  online at s': adv = (1, 3, 4) -> j* = 2
  target at s': adv = (3, 1, 1.25), mean 1.75, val 1.5 -> q = (2.75, 0.75, 1.0):
    the target's own maximum is j = 0 (2.75); double-Q takes q'[2] = 1.0
  y = 0.5 + 0.5 * 1.0 = 1.0; q(s) = (2, 1, 3) - 2 + 1.75 -> q[0] = 1.75;
  td = 0.75; l = 0.5 * 0.75^2 = 0.28125; g = 1 * 0.75 / 2 = 0.375
loss = (0.5 * 4.25 + 0.28125) / 2; mean |td| = (4.75 + 0.75) / 2
d loss / d bA_j = sum_i g_i ([j == a_i] - 1/3); d loss / d bV = sum_i g_i
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def case():
    eye = [[1.0, 0.0], [0.0, 1.0]]
    g0, g1 = 0.25, 0.375
    return {
        'gamma': 0.5, 'hidden': [2], 'A': 3, 'D': 2,
        'q_func': {'fc_action_layers.0.weight': eye, 'fc_action_layers.0.bias': [0.0, 0.0],
                   'fc_action_layers.1.weight': [[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]],
                   'fc_action_layers.1.bias': [0.0, 0.0, 0.0],
                   'fc_state_layers.0.weight': eye, 'fc_state_layers.0.bias': [0.0, 0.0],
                   'fc_state_layers.1.weight': [[0.5, 0.5]], 'fc_state_layers.1.bias': [0.25]},
        'q_target': {'fc_action_layers.0.weight': eye, 'fc_action_layers.0.bias': [0.0, 0.0],
                     'fc_action_layers.1.weight': [[0.0, 1.0], [1.0, 0.0], [0.5, 0.25]],
                     'fc_action_layers.1.bias': [0.0, 0.0, 0.0],
                     'fc_state_layers.0.weight': eye, 'fc_state_layers.0.bias': [0.0, 0.0],
                     'fc_state_layers.1.weight': [[0.25, 0.25]], 'fc_state_layers.1.bias': [0.5]},
        'obs': [[1.0, 2.0], [2.0, 1.0]], 'actions': [2, 0], 'rewards': [-2.0, 0.5],
        'obs_next': [[3.0, 1.0], [1.0, 3.0]], 'dones': [1.0, 0.0], 'weights': [0.5, 1.0],
        'y': [-2.0, 1.0], 'td': [4.75, 0.75],
        'target_own_max': [None, 2.75], 'double_q_value': [None, 1.0],
        'loss': (0.5 * 4.25 + 0.28125) / 2, 'td_error': (4.75 + 0.75) / 2,
        'grad_action_bias': [g1 * (1 - 1 / 3) - g0 / 3, -(g0 + g1) / 3, g0 * (1 - 1 / 3) - g1 / 3],
        'grad_state_bias': [g0 + g1],
    }


if __name__ == '__main__':
    with open(os.path.join(HERE, 'dqn_known_answers.json'), 'w') as f:
        json.dump(case(), f, indent=1)
