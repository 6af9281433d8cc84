defmodule Exmc.NUTS.HipAdviNative do
  @moduledoc """
  NIF binding of `libexmc_hip.so`'s ADVI (`include/exmc_hip_advi.h`, DESIGN.md "ADVI"): `Exmc.ADVI` of a
  built model kind with one mean-field fit per lane group, all fits of a call in one launch. The C side
  is `c_src/exmc_hip_advi_nif.c`, a module beside `Exmc.NUTS.HipPathfinderNative`; conventions are
  HipNative's. `Exmc.NUTS.HipAdvi.fit/2` is the caller.

  Load: `priv/exmc_hip_advi_nif.so` (build line in `INTEGRATION.md`); `EXMC_HIP_DEVICE` selects the GPU.
  """

  @on_load :load_nif

  @doc false
  def load_nif do
    path = :filename.join(:code.priv_dir(:exmc), ~c"exmc_hip_advi_nif")

    case :erlang.load_nif(path, 0) do
      :ok -> :ok
      {:error, _reason} -> :ok
    end
  end

  @doc """
  model = {kind, data_bin} as `HipNative.model_create/2` takes them; perm as `HipNative.model_set_flat_order/2`
  takes it (`[]`: kernel order); fit c runs with seed + 7919 (chain_lo + c) ->
  `{draws [fit][draw][dim], mu [fit][dim], log_sigma [fit][dim], elbo_history [fit][max_iters]}` as f64
  binaries in kernel order and unconstrained space (the history is NaN at and after `num_iters`), then
  `{num_iters, converged}` as i32 binaries `[fit]`, all in one 6-tuple. `lanes` 0 is the kind's default
  layout.
  """
  def fit(_model, _perm, _n_fits, _chain_lo, _num_draws, _max_iters, _num_mc_samples, _window_size,
        _learning_rate, _convergence_tol, _seed, _lanes),
      do: :erlang.nif_error(:nif_not_loaded)
end
