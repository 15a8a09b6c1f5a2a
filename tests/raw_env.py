"""A level-taking env entry point on buffers of the test's own (test_circle_env_gpu.py, test_car_env_gpu.py)."""
import torch

DEV = 'cuda:0'
SENTINEL = -777.0


class RawEnv:
    """An entry point on buffers of the test's own: PAD rows past N and the columns past obs_dim (ld_obs > obs_dim)
    hold a sentinel that every launch must leave alone."""
    PAD = 3

    def __init__(self, entry_point, state_width, level, N, obs_dim, ld, horizon, seed):
        from omnisafe_amd import _lib

        self.lib, self._lib = _lib.load(require_gpu=True), _lib
        self.fn = getattr(self.lib, entry_point)
        self.level, self.N, self.D, self.ld, self.horizon, self.seed = level, N, obs_dim, ld, horizon, seed
        R = N + self.PAD
        f32 = dict(dtype=torch.float32, device=DEV)
        self.state = torch.full((R, state_width), SENTINEL, **f32)
        self.steps = torch.full((R,), 99, dtype=torch.int32, device=DEV)
        self.obs, self.final = torch.full((R, ld), SENTINEL, **f32), torch.full((R, ld), SENTINEL, **f32)
        self.reward, self.cost = torch.full((R,), SENTINEL, **f32), torch.full((R,), SENTINEL, **f32)
        self.term = torch.full((R,), 9, dtype=torch.uint8, device=DEV)
        self.trunc = torch.full((R,), 9, dtype=torch.uint8, device=DEV)
        self.base = torch.zeros(1, dtype=torch.int64, device=DEV)

    def launch(self, pos, action, reset_only, obs_dim=None, state='own'):
        p = self._lib.ptr
        ld_a = action.stride(0) if action is not None else 0
        return self.fn(
            self.seed, pos, p(self.base), self.N, self.D if obs_dim is None else obs_dim, self.horizon, self.level,
            p(self.state) if state == 'own' else None, p(self.steps), p(action), ld_a, p(self.obs), self.ld,
            p(self.reward), p(self.cost), p(self.term), p(self.trunc), p(self.final), self.ld, reset_only,
            self._lib.stream_ptr())

    def pads_untouched(self):
        N, D = self.N, self.D
        ok = bool((self.state[N:] == SENTINEL).all()) and bool((self.steps[N:] == 99).all())
        for rows in (self.obs, self.final):
            ok = ok and bool((rows[N:] == SENTINEL).all()) and bool((rows[:, D:] == SENTINEL).all())
        ok = ok and bool((self.reward[N:] == SENTINEL).all()) and bool((self.cost[N:] == SENTINEL).all())
        return ok and bool((self.term[N:] == 9).all()) and bool((self.trunc[N:] == 9).all())
