"""The oracle environment on rectangular worlds (no GPU).

The reference is square (``% self.dim``); ``OracleDaisyWorld.set_initial_cover`` accepts H x W covers and the agents'
code then wraps rows by H and columns by W.  Nothing but the library itself had ever been compared with a non-square
world with agents, so the generalisation is pinned here by properties that need no second implementation:

  (a) on a square world the ``set_initial_cover`` path is the existing one (grid, agents, obs, reward, done);
  (b) the model has no preferred axis: an (H, W) run equals the (W, H) run of the transposed state with the move
      codes mirrored (left <-> up, down <-> right; code 5 has no mirror image and is left to the GPU tests);
  (c) an agent stepping over the last row / column lands on row / column 0.
"""
import numpy as np
import pytest

from oracle import daisy_oracle as O

ENVS = [O.OracleDaisyWorld, O.OracleDaisyWorldC]


def _k(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def _covers(rng, B, H, W):
    """Covers as initialize_grid draws them (ref :285-303), for any H x W."""
    dark_prob, light_prob = rng.rand(B, 2, H, W), rng.rand(B, 2, H, W)
    dark = 1.0 * (dark_prob[:, 0] < 0.33) * 0.2 * dark_prob[:, 1]
    light = 1.0 * (light_prob[:, 0] < 0.33) * 0.2 * light_prob[:, 1]
    return light, dark


def _world(cls, B, H, W, N, light, dark, idx, L=0.9):
    env = cls(grid_dimension=max(H, W), n_agents=N, batch_size=B)
    env.L = L
    env.set_initial_cover(light, dark)
    env.agent_indices = np.array(idx, dtype=np.int64).reshape(B, N, 2)
    env.agent_states = np.ones((B, N, 1))
    return env


# ---- (a) square: set_initial_cover == the existing path -------------------------------------------------------------
@pytest.mark.parametrize("cls", ENVS)
def test_square_world_through_set_initial_cover_equals_reset_path(cls):
    B, G, N, K = 3, 8, 4, 12
    np.random.seed(11)
    a = cls(grid_dimension=G, n_agents=N, batch_size=B)
    obs_a = a.reset()                                           # initialize_grid -> set_initial_cover, initialize_agents
    b = cls(grid_dimension=G, n_agents=N, batch_size=B)
    b.L = a.L
    b.set_initial_cover(a.grid[:, O.CH_LIGHT].copy(), a.grid[:, O.CH_DARK].copy())
    b.agent_indices = a.agent_indices.copy()
    b.agent_states = a.agent_states.copy()
    assert b.shape == (G, G) and np.array_equal(a.grid, b.grid)
    assert np.array_equal(obs_a, b.get_obs(b.agent_indices))
    rng = np.random.RandomState(5)
    for t in range(K):
        act = rng.randint(9, size=(B, N, 1))
        oa, ra, da, _ = a.step(act.copy())
        ob, rb, db, _ = b.step(act.copy())
        assert np.array_equal(a.grid, b.grid), t
        assert np.array_equal(a.agent_indices, b.agent_indices) and np.array_equal(a.agent_states, b.agent_states), t
        assert np.array_equal(oa, ob) and np.array_equal(ra, rb) and np.array_equal(da, db), t
        assert a.L == b.L
    assert (a.agent_states < 1.0).any()


def test_square_world_wraps_by_dim_as_before():
    """The square wrap, spelled out against the reference's own arithmetic (% dim, ref :208,259-260)."""
    G = 5
    light, dark = _covers(np.random.RandomState(1), 1, G, G)
    env = _world(O.OracleDaisyWorld, 1, G, G, 2, light, dark, [[G - 1, 0], [0, G - 1]])
    obs = env.get_obs(env.agent_indices)
    rows = (np.array([G - 1, 0])[:, None] + np.arange(-1, 2)) % G
    cols = (np.array([0, G - 1])[:, None] + np.arange(-1, 2)) % G
    for n in range(2):
        assert np.array_equal(obs[0, n], env.grid[0][:, rows[n]][:, :, cols[n]] * env.neighborhood)
    env.step(np.array([[[2], [3]]]))                            # down from the last row, right from the last column
    assert np.array_equal(env.agent_indices[0], [[0, 0], [0, 0]])


# ---- (b) transposition ----------------------------------------------------------------------------------------------
# move codes a % 4: 0 = column - 1, 1 = row - 1, 2 = row + 1, 3 = column + 1 (ref :196-207); transposing the world
# swaps rows and columns: 0 <-> 1, 2 <-> 3, 6 <-> 7; 8 stays.  Grazing is `a > 4` (ref :210), so 4 is a plain move to
# the left like 0 and goes to 1, and 5 - up AND graze - has no counterpart (left and graze would be 8, which stays): the
# (H, W) run draws from every code but 5, the transposed run then takes neither 4 nor 5.
CODES = np.array([0, 1, 2, 3, 4, 6, 7, 8])
T_CODE = np.array([1, 0, 3, 2, 1, -1, 7, 6, 8])


@pytest.mark.parametrize("cls", ENVS)
@pytest.mark.parametrize("shape", [(3, 5), (7, 9), (4, 64)])
def test_rectangular_run_equals_transposed_run(cls, shape):
    H, W = shape
    B, N, K = 2, 4, 12
    rng = np.random.RandomState(H * 100 + W)
    light, dark = _covers(rng, B, H, W)
    idx = np.stack([rng.randint(H, size=(B, N)), rng.randint(W, size=(B, N))], axis=-1)
    idx[0, 1] = idx[0, 0]                                       # two agents on one cell from the start
    a = _world(cls, B, H, W, N, light, dark, idx)
    b = _world(cls, B, W, H, N, np.ascontiguousarray(light.transpose(0, 2, 1)),
               np.ascontiguousarray(dark.transpose(0, 2, 1)), idx[..., ::-1])
    assert a.shape == (H, W) and b.shape == (W, H)
    table = CODES[rng.randint(CODES.size, size=(K, B, N, 1))]
    assert set(np.unique(table)) == set(CODES)
    table[:3, 0, :2] = 7                                        # ... that graze the same cells: order decides who eats
    L, ate = 0.9, False
    for t in range(K):
        a.L = b.L = L
        before = a.agent_states.copy()
        oa, ra, da, _ = a.step(table[t].copy())
        ob, rb, db, _ = b.step(T_CODE[table[t]])
        L += 0.004
        assert np.array_equal(_k(a.grid[:, 1]), _k(b.grid[:, 1]).transpose(0, 2, 1)), t
        assert np.array_equal(_k(a.grid[:, 2]), _k(b.grid[:, 2]).transpose(0, 2, 1)), t
        assert np.array_equal(a.agent_indices, b.agent_indices[..., ::-1]), t
        assert np.array_equal(a.agent_states, b.agent_states), t
        ate = ate or bool((a.agent_states > before - a.P.agent_gamma).any())
        assert np.array_equal(ra, rb) and np.array_equal(da, db), t
        # observations: light, dark and the agents' stamps (channel 4 at stamped cells is a state) transpose exactly;
        # the un-stamped temperatures are rounded sums whose order of addition the transposition changes
        assert np.array_equal(_k(oa[:, :, 1:3]), _k(ob[:, :, 1:3]).transpose(0, 1, 2, 4, 3)), t
    assert ate and (a.agent_states < 1.0).any() and (a.agent_indices != idx).any()      # the run grazed, starved, moved


# ---- (c) edge wrap on a wide, flat world ----------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ENVS)
def test_agents_wrap_by_rows_and_by_columns_on_3x85(cls):
    H, W = 3, 85
    light, dark = _covers(np.random.RandomState(2), 1, H, W)
    # agent 0: last row, moving down; agent 1: last column, moving right; agent 2 / 3: row 0 up, column 0 left
    env = _world(cls, 1, H, W, 4, light, dark, [[H - 1, 40], [1, W - 1], [0, 70], [2, 0]])
    obs = env.get_obs(env.agent_indices)
    g = env.grid[0]
    assert np.array_equal(obs[0, 0, :, 2, 1], g[:, 0, 40])      # below the last row: row 0
    assert np.array_equal(obs[0, 1, :, 1, 2], g[:, 1, 0])       # right of the last column: column 0
    assert np.array_equal(obs[0, 2, :, 0, 1], g[:, H - 1, 70])
    assert np.array_equal(obs[0, 3, :, 1, 0], g[:, 2, W - 1])
    env.step(np.array([[[2], [3], [1], [0]]]))
    assert np.array_equal(env.agent_indices[0], [[0, 40], [1, 0], [H - 1, 70], [2, W - 1]])
    env.step(np.array([[[5], [4], [6], [7]]]))                  # and back over the same edges, grazing
    assert np.array_equal(env.agent_indices[0], [[H - 1, 40], [1, W - 1], [0, 70], [2, 0]])
    assert env.agent_indices[..., 0].max() < H and env.agent_indices[..., 1].max() < W


def test_collisions_iterate_the_grids_own_shape():
    """collision_mode 1 on 3 x 85: two agents meeting at column 84 (beyond a 3 x 3 scan) are found, and exactly one jitter block is drawn."""
    H, W = 3, 85
    light, dark = _covers(np.random.RandomState(3), 1, H, W)
    env = O.OracleDaisyWorld(grid_dimension=H, n_agents=3, batch_size=1, collision_mode=1)
    env.L = 0.9
    env.set_initial_cover(light, dark)
    env.agent_indices = np.array([[[2, 0], [2, 0], [0, 3]]], dtype=np.int64)
    env.agent_states = np.array([[[0.9], [0.4], [0.7]]])
    np.random.seed(4)
    env.step(np.full((1, 3, 1), 0))                             # a plain move to the left: nobody grazes
    after = np.random.rand()
    np.random.seed(4)
    np.random.rand(1, 3, 1)
    assert after == np.random.rand()                            # one draw of the (1, N, 1) block
    assert np.array_equal(env.agent_indices[0], [[2, 84], [2, 84], [0, 2]])
    g = env.P.agent_gamma
    assert env.agent_states[0, 0, 0] == min(1.0, (0.9 - g) + 0.5 * (0.4 - g))     # the winner eats half the loser's state
    assert env.agent_states[0, 1, 0] == 0.4 - g and env.agent_states[0, 2, 0] == 0.7 - g
