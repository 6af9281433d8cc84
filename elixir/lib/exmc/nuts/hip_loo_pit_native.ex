defmodule Exmc.NUTS.HipLooPitNative do
  @moduledoc """
  NIF binding of `libexmc_hip.so`'s PSIS-LOO-PIT (`include/exmc_hip_loo_pit.h`, DESIGN.md "LOO-PIT"): the
  replicates of `Exmc.NUTS.HipPredictiveNative` weighted on the device with the Pareto-smoothed
  leave-one-out weights of PSIS-LOO, neither matrix kept. The C side is `c_src/exmc_hip_loo_pit_nif.c`, a
  module beside `Exmc.NUTS.HipPpcNative`; conventions are HipNative's. `Exmc.NUTS.HipLooPit.loo_pit/3` is
  the caller.

  Load: `priv/exmc_hip_loo_pit_nif.so` (build line in `INTEGRATION.md`); `EXMC_HIP_DEVICE` selects the GPU.
  """

  @on_load :load_nif

  @doc false
  def load_nif do
    path = :filename.join(:code.priv_dir(:exmc), ~c"exmc_hip_loo_pit_nif")

    case :erlang.load_nif(path, 0) do
      :ok -> :ok
      {:error, _reason} -> :ok
    end
  end

  @doc """
  model = {kind, data_bin} as `HipNative.model_create/2` takes them; draws: `[chain][draw][dim]` f64
  binary in kernel order; chain c draws with seed + 7919 (chain_lo + c) ->
  `out_bin [4][datum]`, an f64 binary: the rows p_lt, p_eq, pit and the Pareto k, the datums in the kind's
  data order
  """
  def loo_pit(_model, _draws, _n_chains, _n_draws, _seed, _chain_lo),
    do: :erlang.nif_error(:nif_not_loaded)
end
