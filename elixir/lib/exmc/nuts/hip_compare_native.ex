defmodule Exmc.NUTS.HipCompareNative do
  @moduledoc """
  NIF binding of `libexmc_hip.so`'s model comparison (`include/exmc_hip_compare.h`): the per-datum
  statistics of `Exmc.ModelComparison` for a built model kind, computed on the device. The C side is
  `c_src/exmc_hip_compare_nif.c` (a module of its own next to `Exmc.NUTS.HipNative`, whose table it
  leaves as it is); conventions are HipNative's.

  Load: `priv/exmc_hip_compare_nif.so` (build line in `INTEGRATION.md`); `EXMC_HIP_DEVICE` selects the GPU.
  """

  @on_load :load_nif

  @doc false
  def load_nif do
    path = :filename.join(:code.priv_dir(:exmc), ~c"exmc_hip_compare_nif")

    case :erlang.load_nif(path, 0) do
      :ok -> :ok
      {:error, _reason} -> :ok
    end
  end

  @doc """
  model = {kind, data_bin} as `HipNative.model_create/2` takes them; draws: `[chain][draw][dim]` f64
  binary in kernel order, as HipNative's sampling functions return it -> `[4][N]` f64 binary, rows lppd,
  p_waic, elpd_loo, p_loo (datums in the kind's data order)
  """
  def ic_stats(_model, _draws, _n_chains, _n_draws), do: :erlang.nif_error(:nif_not_loaded)
end
