"""Host tests of the settings table (mvus_amd.reconstruction.ba_settings), of BAHandle.configure against a stand-in library, and of the
layout of the camera-side head of x (mvus_amd.problem.HeadLayout).  No GPU, no libmvusba.so."""
import numpy as np
import pytest

from mvus_amd import _lib, ba, problem
from mvus_amd.reconstruction import ba_settings, common

NAMES = "['alpha', 'beta', 'rs', 'R', 't', 'K', 'd']"

# one value of the wrong type or range for every key of the table that is validated
BAD = {'ba_solver': 'newton', 'ba_jacobian': 'exact', 'ba_loss': 'tukey', 'ba_f_scale': 0.0, 'ba_gauge': 'fixed', 'ba_freeze': [0],
       'ba_covariance': 1, 'ba_kinematics': 'yes', 'ba_detection_covariance': 0, 'ba_register': 'true', 'ba_register_beta_search': [1.0],
       'ba_position_priors': 1, 'ba_landmarks': 'on'}
UNVALIDATED = {'ba_lambda_min', 'ba_trust_radius', 'ba_lm_wide_band', 'ba_pattern_ties', 'ba_deterministic'}


def _scene(**settings):
    s = common.Scene()
    s.settings = dict(settings)
    return s


def test_the_table_lists_every_key():
    assert set(ba_settings.KEYS) == set(BAD) | UNVALIDATED
    assert {k for k, row in ba_settings.KEYS.items() if row.check is None} == UNVALIDATED
    assert all(row.doc.strip() for row in ba_settings.KEYS.values())


@pytest.mark.parametrize('key', [k for k, row in ba_settings.KEYS.items() if row.check is not None])
def test_ba_mode_reaches_every_validated_key(key, monkeypatch):
    """A bad value under any key of the table that is not marked there as unvalidated makes ``Scene.ba_mode()`` raise, naming the key,
    and no handle is made."""
    def no_handle(self, prob):
        raise AssertionError('reached the library with bad settings')
    monkeypatch.setattr(common.Scene, '_handle', no_handle)
    s = _scene(ba_solver='lm', opt_calib=False)
    assert s.ba_mode() == (ba.SOLVER_LM_SCHUR, ba.JAC_ANALYTIC)
    s.settings[key] = BAD[key]
    with pytest.raises(ValueError, match=r"settings\['%s'\]" % key):
        s.ba_mode()


FLAGS = [('ba_covariance', 'ba_covariance_enabled'), ('ba_kinematics', 'ba_kinematics_enabled'),
         ('ba_detection_covariance', 'ba_detection_covariance_enabled'), ('ba_register', 'ba_register_enabled'),
         ('ba_landmarks', 'ba_landmarks'), ('ba_position_priors', 'ba_position_priors')]

# (settings, the Scene reader that raises, its message): the strings of the readers as they stood in common.py before the table
MESSAGES = [
    (dict(ba_solver='newton'), 'ba_mode', "settings['ba_solver'] must be 'trf' or 'lm', not 'newton'"),
    (dict(ba_jacobian='exact'), 'ba_mode', "settings['ba_jacobian'] must be one of ['analytic', 'fd', 'pattern'], not 'exact'"),
    (dict(ba_loss='tukey'), 'ba_loss', "settings['ba_loss'] must be one of ['arctan', 'cauchy', 'huber', 'linear', 'soft_l1'], not 'tukey'"),
    (dict(ba_loss=2), 'ba_loss', "settings['ba_loss'] must be one of ['arctan', 'cauchy', 'huber', 'linear', 'soft_l1'], not 2"),
    (dict(ba_f_scale=0.0), 'ba_loss', "settings['ba_f_scale'] must be a finite positive number, not 0.0"),
    (dict(ba_f_scale=True), 'ba_loss', "settings['ba_f_scale'] must be a finite positive number, not True"),
    (dict(ba_loss='huber'), 'ba_loss',
     "settings['ba_loss'] = 'huber' needs settings['ba_solver'] = 'lm' (the TRF + LSMR solver has no robust loss), not 'trf'"),
    (dict(ba_solver='lm', ba_jacobian='pattern', ba_loss='huber'), 'ba_loss',
     "settings['ba_loss'] = 'huber' needs settings['ba_jacobian'] = 'analytic', not 'pattern'"),
    (dict(ba_gauge='fixed'), 'ba_freeze', "settings['ba_gauge'] must be 'free' or 'anchor', not 'fixed'"),
    (dict(ba_freeze=[0]), 'ba_freeze', "settings['ba_freeze'] must map camera indices to lists of names from %s, not [0]" % NAMES),
    (dict(ba_freeze={'a': ['R']}), 'ba_freeze', "settings['ba_freeze']: 'a' is not a camera index"),
    (dict(ba_freeze={1.0: ['R']}), 'ba_freeze', "settings['ba_freeze']: 1.0 is not a camera index"),
    (dict(ba_freeze={-1: ['R']}), 'ba_freeze', "settings['ba_freeze']: -1 is not a camera index"),
    (dict(ba_freeze={'0': 'R'}), 'ba_freeze', "settings['ba_freeze']['0'] must be a list of names from %s, not 'R'" % NAMES),
    (dict(ba_freeze={'0': ['q']}), 'ba_freeze', "settings['ba_freeze']['0']: unknown name 'q' (one of %s)" % NAMES),
    (dict(ba_freeze={'0': ['K']}), 'ba_freeze',
     "settings['ba_freeze']['0']: 'K' is a parameter only with settings['opt_calib'] (fixed calibration is not in x)"),
    (dict(ba_register_beta_search=[1.0]), 'ba_register_beta_search',
     "settings['ba_register_beta_search'] must be [half_width, step] in frames (finite, half_width >= 0, step > 0), not [1.0]"),
    (dict(ba_register_beta_search=[2, 0]), 'ba_register_beta_search',
     "settings['ba_register_beta_search'] must be [half_width, step] in frames (finite, half_width >= 0, step > 0), not [2, 0]"),
    (dict(ba_landmarks=True), 'ba_landmarks',
     "settings['ba_landmarks'] needs settings['ba_solver'] = 'lm' (the TRF + LSMR solver takes no landmarks), not 'trf'"),
    (dict(ba_position_priors=True, ba_solver='trf'), 'ba_position_priors',
     "settings['ba_position_priors'] needs settings['ba_solver'] = 'lm' (the TRF + LSMR solver takes no position priors), not 'trf'"),
    (dict(traj_weights='gps'), 'traj_weights', "settings['traj_weights'] must be 'triangulation' or absent, not 'gps'"),
    (dict(traj_weights='triangulation', traj_sigma_px=-1.0), 'traj_weights', "settings['traj_sigma_px'] must be a positive number, or one per camera"),
    (dict(traj_weights='triangulation', traj_weight_floor=2.0), 'traj_weights', "settings['traj_weight_floor'] must lie in (0, 1]"),
] + [({key: 'yes'}, reader, "settings['%s'] must be true or false, not 'yes'" % key) for key, reader in FLAGS]


@pytest.mark.parametrize('settings,reader,message', MESSAGES)
def test_messages_are_what_they_were(settings, reader, message):
    s = _scene(**settings)
    with pytest.raises(ValueError) as e:
        getattr(s, reader)()
    assert str(e.value) == message
    if reader != 'traj_weights':                 # (ba_mode never validated traj_weights and does not start to)
        with pytest.raises(ValueError) as e:
            s.ba_mode()
        assert str(e.value) == message
    else:
        assert s.ba_mode() == (ba.SOLVER_TRF_LSMR, ba.JAC_FD)


def test_the_first_bad_key_is_the_one_it_was():
    """Two bad keys: the one the readers met first in the old ``ba_mode`` still raises first."""
    order = ['ba_solver', 'ba_jacobian', 'ba_loss', 'ba_f_scale', 'ba_gauge', 'ba_freeze', 'ba_covariance', 'ba_kinematics',
             'ba_detection_covariance', 'ba_register', 'ba_register_beta_search', 'ba_position_priors', 'ba_landmarks']
    assert [k for k, row in ba_settings.KEYS.items() if row.check is not None] == order
    for first, second in zip(order, order[1:]):
        s = _scene(**{'ba_solver': 'lm', first: BAD[first], second: BAD[second]})
        with pytest.raises(ValueError, match=r"settings\['%s'\]" % first):
            s.ba_mode()


def test_a_bad_array_still_raises_from_ba_mode():
    s = _scene(ba_solver='lm', ba_position_priors=True)
    s.position_priors = np.ones((6, 3))
    with pytest.raises(ValueError, match=r'Scene.position_priors must be a \(7, K\) array'):
        s.ba_mode()
    s = _scene(ba_solver='lm', ba_landmarks=True)
    s.landmarks, s.landmark_observations = np.zeros((3, 2)), np.array([[0.0], [5.0], [1.0], [1.0], [1.0], [1.0]])
    with pytest.raises(ValueError, match=r'Scene.landmarks: camera ids must be whole'):
        s.ba_mode()


def test_settings_that_are_no_dict_give_the_defaults():
    s = common.Scene()
    assert s.settings == [] and ba_settings.as_dict(s.settings) == {}
    assert s.ba_mode() == (ba.SOLVER_TRF_LSMR, ba.JAC_FD)
    assert s.ba_loss() == (ba.LOSS_LINEAR, 1.0)
    assert s.ba_freeze() == ({}, 'free')
    for _, reader in FLAGS[:4]:
        assert getattr(s, reader)() is False
    assert s.ba_register_beta_search() is None and s.ba_landmarks() is None and s.ba_position_priors() is None and s.traj_weights() is None


def test_solve_options_are_the_librarys_with_the_two_keys_over_them():
    base = _lib.default_opts(ba.SOLVER_LM_SCHUR, ba.JAC_ANALYTIC, 7)
    o = ba_settings.solve_options({}, ba.SOLVER_LM_SCHUR, ba.JAC_ANALYTIC, 7)
    assert (o.solver, o.jac_mode, o.max_nfev, o.lm_lambda_min, o.lm_trust_radius) == \
           (base.solver, base.jac_mode, 7, base.lm_lambda_min, base.lm_trust_radius)
    o = ba_settings.solve_options({'ba_lambda_min': 0.3, 'ba_trust_radius': 2}, ba.SOLVER_LM_SCHUR, ba.JAC_ANALYTIC, 7)
    assert (o.lm_lambda_min, o.lm_trust_radius) == (0.3, 2.0)


# ---- BAHandle.configure against a stand-in library ----------------------------------------------------------------------------------
class FakeLib:
    """Records every mvus_ba_set_* call as (what, distinguishing value) and answers the counts from what was set."""

    def __init__(self):
        self.calls, self.fail = [], 0
        self.frozen = self.priors = self.marks = 0

    def _refused(self):
        if self.fail:
            self.fail -= 1
            return True
        return False

    def mvus_ba_set_loss(self, h, code, f_scale):
        if self._refused():
            return _lib.MVUS_E_INVALID
        self.calls.append(('loss', (code, f_scale)))
        return 0

    def mvus_ba_set_frozen(self, h, mask, n):
        if self._refused():
            return _lib.MVUS_E_INVALID
        bits = [int(mask[i]) for i in range(n)]
        self.frozen = sum(bits)
        self.calls.append(('frozen', bits))
        return 0

    def mvus_ba_set_position_priors(self, h, K, t, P, w):
        if self._refused():
            return _lib.MVUS_E_INVALID
        self.priors = K
        self.calls.append(('priors', [1.0 / w[i] for i in range(3 * K)]))
        return 0

    def mvus_ba_set_landmarks(self, h, L, X, K, cam, point, uv, w):
        if self._refused():
            return _lib.MVUS_E_INVALID
        self.marks = K
        self.calls.append(('landmarks', [uv[i] for i in range(2 * K)]))
        return 0

    def mvus_ba_num_frozen(self, h):
        return self.frozen

    def mvus_ba_num_position_priors(self, h, active):
        return self.priors

    def mvus_ba_num_landmark_observations(self, h, rows):
        return self.marks

    def mvus_last_error(self, h):
        return b'refused by the stand-in'

    def mvus_ba_destroy(self, h):
        pass

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _handle():
    h = ba.BAHandle.__new__(ba.BAHandle)
    h.lib, h.h = FakeLib(), 1
    return h


def _state():
    mask = np.zeros(2 * 9, dtype=bool)
    mask[[0, 7]] = True
    priors = (np.array([1.0, 2.0]), np.arange(6.0).reshape(3, 2), np.full((3, 2), 0.5))
    marks = (np.arange(9.0).reshape(3, 3), np.array([0, 1], dtype=np.int32), np.array([2, 0], dtype=np.int32),
             np.array([[10.0, 20.0], [30.0, 40.0]]), np.ones((2, 2)))
    return dict(loss=(ba.LOSS_HUBER, 2.0), frozen=mask, position_priors=priors, landmarks=marks)


def _copy(state):
    return {k: (v.copy() if isinstance(v, np.ndarray) else tuple(a.copy() if isinstance(a, np.ndarray) else a for a in v)) for k, v in state.items()}


def test_configure_sends_each_state_once_and_in_order():
    h, st = _handle(), _state()
    assert h.loss == (ba.LOSS_LINEAR, 1.0) and h.frozen is None and h.position_priors is None and h.landmarks is None
    h.configure(**st)                                                            # (i)
    assert [c[0] for c in h.lib.take()] == ['loss', 'frozen', 'priors', 'landmarks']
    h.configure(**_copy(st))                                                     # (ii) equal arrays in other objects: nothing to send
    assert h.lib.take() == []
    assert h.loss == st['loss'] and np.array_equal(h.frozen, st['frozen'])
    assert all(np.array_equal(a, b) for a, b in zip(h.position_priors, st['position_priors']))
    assert all(np.array_equal(a, b) for a, b in zip(h.landmarks, st['landmarks']))


def test_configure_sends_exactly_what_changed():
    h, st = _handle(), _state()
    h.configure(**st)
    h.lib.take()
    st = _copy(st)                                                               # (iii)
    st['loss'] = (ba.LOSS_HUBER, 2.5)
    h.configure(**st)
    assert h.lib.take() == [('loss', (ba.LOSS_HUBER, 2.5))]
    st['frozen'][3] = True
    h.configure(**st)
    assert h.lib.take() == [('frozen', [int(b) for b in st['frozen']])]
    st['position_priors'][2][1, 0] = 0.25
    h.configure(**st)
    assert h.lib.take() == [('priors', [0.5, 0.5, 0.25, 0.5, 0.5, 0.5])]
    st['landmarks'][3][0, 1] = 21.0
    h.configure(**st)
    assert h.lib.take() == [('landmarks', [10.0, 21.0, 30.0, 40.0])]
    h.configure(**st)
    h.configure()                                                                # nothing passed: nothing touched
    h.configure(frozen=st['frozen'])
    assert h.lib.take() == []


def test_configure_clears_with_none_only_what_is_in_force():
    h, st = _handle(), _state()
    h.configure(frozen=None, position_priors=None, landmarks=None)               # (iv) nothing in force
    h.configure(frozen=np.zeros(18, dtype=bool))                                 # (v) all false = no mask
    assert h.lib.take() == []
    h.configure(**st)
    h.lib.take()
    h.configure(frozen=None)
    assert h.lib.take() == [('frozen', [])] and h.frozen is None
    h.configure(position_priors=None)
    assert h.lib.take() == [('priors', [])] and h.position_priors is None
    h.configure(landmarks=None)
    assert h.lib.take() == [('landmarks', [])] and h.landmarks is None
    assert h.loss == st['loss']                                                  # not passed: left alone
    h.configure(**st)
    h.lib.take()
    h.configure(frozen=np.zeros(18, dtype=bool))                                 # all false against a mask in force: one call
    assert [c[0] for c in h.lib.take()] == ['frozen'] and h.frozen is None


def test_configure_after_a_direct_set_puts_its_own_rows_back():
    h, st = _handle(), _state()
    h.configure(**st)
    other = _copy(st)['landmarks']                                               # (vi) same size, other pixels
    other[3][:] += 5.0
    h.set_landmarks(*other)
    assert np.array_equal(h.landmarks[3], other[3])
    h.lib.take()
    h.configure(landmarks=st['landmarks'])
    assert h.lib.take() == [('landmarks', [10.0, 20.0, 30.0, 40.0])]
    moved = _copy(st)['position_priors']
    moved[1][:] += 1.0
    h.set_position_priors(*moved)
    h.lib.take()
    h.configure(position_priors=st['position_priors'])
    assert [c[0] for c in h.lib.take()] == ['priors'] and np.array_equal(h.position_priors[1], st['position_priors'][1])


def test_a_refused_set_leaves_the_record():
    h, st = _handle(), _state()                                                  # (vii)
    h.configure(**st)
    other = _copy(st)
    other['landmarks'][3][:] += 5.0
    other['position_priors'][1][:] += 1.0
    for call in (lambda: h.set_loss('cauchy', 3.0), lambda: h.set_frozen(np.ones(18, dtype=bool)), lambda: h.set_frozen(None),
                 lambda: h.set_landmarks(*other['landmarks']), lambda: h.set_landmarks(None, None, None, None, None),
                 lambda: h.set_position_priors(*other['position_priors']), lambda: h.set_position_priors(None, None, None)):
        h.lib.fail = 1
        with pytest.raises(ValueError, match='refused by the stand-in'):
            call()
    assert h.loss == st['loss'] and np.array_equal(h.frozen, st['frozen'])
    assert np.array_equal(h.landmarks[3], st['landmarks'][3]) and np.array_equal(h.position_priors[1], st['position_priors'][1])
    h.lib.take()
    h.configure(**st)
    assert h.lib.take() == []


# ---- the head of x ------------------------------------------------------------------------------------------------------------------
NAMES6 = ['r1', 'r2', 'r3', 't1', 't2', 't3']
NAMES15 = ['fx', 'fy', 'cx', 'cy', 'r1', 'r2', 'r3', 't1', 't2', 't3', 'k1', 'k2', 'p1', 'p2', 'k3']


@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('calib', [False, True])
def test_head_layout(calib, C):
    lay = problem.HeadLayout(calib, C)
    names = NAMES15 if calib else NAMES6
    assert lay.names == names and lay.P == len(names) and lay.size == C * (3 + len(names))
    assert _scene(opt_calib=calib).ba_param_names() == names
    parts = {'K': [0, 1, 2, 3], 'R': [4, 5, 6], 't': [7, 8, 9], 'd': [10, 11, 12, 13, 14]} if calib else {'R': [0, 1, 2], 't': [3, 4, 5]}
    assert {k: list(v) for k, v in lay.part.items()} == parts
    seen = []
    for k in range(C):
        assert [lay.index(k, n) for n in ('alpha', 'beta', 'rs')] == [k, C + k, 2 * C + k]
        assert [lay.index(k, n) for n in names] == [lay.index(k, j) for j in range(lay.P)] == list(range(3 * C + k * lay.P, 3 * C + (k + 1) * lay.P))
        for group, js in parts.items():
            assert lay.indices(k, group) == [3 * C + k * lay.P + j for j in js]
        seen += [lay.index(k, n) for n in ('alpha', 'beta', 'rs')] + [lay.index(k, j) for j in range(lay.P)]
    assert sorted(seen) == list(range(lay.size))


def _posed_scene(C, **settings):
    s = _scene(**settings)
    for k in range(C):                           # camera 1: R_1 (C_0 - C_1) = t_1 - t_0 = (-1, -5, 2), largest in component 1
        s.addCamera(common.Camera(K=np.eye(3), d=np.zeros(5), R=np.eye(3), t=np.array([-1.0, -5.0, 2.0]) * k))
    return s


def test_frozen_mask_by_hand():
    free = dict(ba_freeze={'0': ['alpha', 'R'], '1': ['t', 'rs']})
    mask = _posed_scene(2, opt_calib=False, **free).ba_frozen_mask([0, 1])
    assert mask.size == 18 and set(np.nonzero(mask)[0]) == {0, 5, 6, 7, 8, 15, 16, 17}
    mask = _posed_scene(2, opt_calib=False, ba_gauge='anchor', **free).ba_frozen_mask([0, 1])
    assert set(np.nonzero(mask)[0]) == {0, 5, 6, 7, 8, 9, 10, 11, 15, 16, 17}
    mask = _posed_scene(3, opt_calib=False, ba_gauge='anchor').ba_frozen_mask([0, 1, 2])
    assert mask.size == 27 and set(np.nonzero(mask)[0]) == {9, 10, 11, 12, 13, 14, 19}
    calib = dict(ba_freeze={'0': ['alpha', 'K'], '1': ['d', 'rs']}, opt_calib=True)
    mask = _posed_scene(2, **calib).ba_frozen_mask([0, 1])
    assert mask.size == 36 and set(np.nonzero(mask)[0]) == {0, 5, 6, 7, 8, 9, 31, 32, 33, 34, 35}
    mask = _posed_scene(2, ba_gauge='anchor', **calib).ba_frozen_mask([0, 1])
    assert set(np.nonzero(mask)[0]) == {0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 29, 31, 32, 33, 34, 35}
    mask = _posed_scene(3, **calib).ba_frozen_mask([2, 1])                        # camera 1 stands second: k = 1 of C = 2; camera 0 is not in
    assert set(np.nonzero(mask)[0]) == {5, 31, 32, 33, 34, 35}
