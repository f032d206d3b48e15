'use strict';
/* The cluster pair schedule through the JavaScript facade, shared by tests/js/pairs_cluster_cpu.js (oracle-backed mock addon) and
 * tests/js/pairs_cluster_gpu.js (product addon on a GPU): tests/js/pairs_common.js — the batch part, the per-feed-state loop and
 * camshift.MultiTracker, with the expectations of the existing pairs job — run with every DeviceBatch created with
 * {pairSchedule: 'cluster'} and headtrackr.camshift.pairSchedule = 'cluster'.  `A` is the addon object the facade uses; its createContext
 * is wrapped to record the config objects it receives (out.created). */
const path = require('path');

module.exports = function run(A, headtrackr, Canvas, job, out, check) {
  out.created = [];
  const realCreate = A.createContext;
  A.createContext = function (cfg) { out.created.push(cfg && Object.prototype.hasOwnProperty.call(cfg, 'options') ? cfg.options : null); return realCreate.apply(this, arguments); };

  /* the option values: anything but the two names is a RangeError, before a context is created */
  const J = job.loop;
  ['Cluster', '', 1, null].forEach(function (v) {
    let threw = false;
    try { new headtrackr.ccv.DeviceBatch(J.w, J.h, J.n, { depth: 1, pairSchedule: v }); } catch (e) { threw = e instanceof RangeError; }
    check(threw, 'DeviceBatch pairSchedule ' + JSON.stringify(v) + ' must be a RangeError');
  });
  let threw = false;
  try { headtrackr.camshift.pairSchedule = 'clusters'; } catch (e) { threw = e instanceof RangeError; }
  check(threw && headtrackr.camshift.pairSchedule === 'workgroup', "camshift.pairSchedule = 'clusters' must be a RangeError and change nothing");
  check(out.created.length === 0, 'a refused value creates no context');

  /* default and explicit 'workgroup': no options key at all; 'cluster': the option, for every context of the batch */
  [[undefined, 2], ['workgroup', 1], ['cluster', 3]].forEach(function (c) {
    const before = out.created.length, opts = { depth: c[1] };
    if (c[0] !== undefined) opts.pairSchedule = c[0];
    const b = new headtrackr.ccv.DeviceBatch(J.w, J.h, J.n, opts);
    const mine = out.created.slice(before);
    check(b.pairSchedule === (c[0] || 'workgroup'), 'DeviceBatch.pairSchedule is ' + b.pairSchedule);
    check(mine.length === c[1] && mine.every(function (o) { return o === (c[0] === 'cluster' ? 'cs_pairs_cluster=1' : null); }),
      'DeviceBatch ' + JSON.stringify(opts) + ' created contexts with options ' + JSON.stringify(mine));
    b.destroy();
  });
  out.option_checks = out.created.length;

  /* the existing pairs job on the cluster schedule */
  const Real = headtrackr.ccv.DeviceBatch;
  headtrackr.ccv.DeviceBatch = function (w, h, n, opts) { return new Real(w, h, n, Object.assign({}, opts, { pairSchedule: 'cluster' })); };
  headtrackr.camshift.pairSchedule = 'cluster';
  check(headtrackr.camshift.pairSchedule === 'cluster' && headtrackr.camshift._pool.ctx === null, 'camshift.pairSchedule is taken before the pool exists');
  const before = out.created.length;
  require(path.join(__dirname, 'pairs_common.js'))(headtrackr, Canvas, job, out, check);
  headtrackr.ccv.DeviceBatch = Real;
  const mine = out.created.slice(before);
  check(mine.length === 3 && mine.every(function (o) { return o === 'cs_pairs_cluster=1'; }),
    'two DeviceBatch contexts and the camshift pool context carry the option: ' + JSON.stringify(mine));
  out.job_contexts = mine.length;

  /* the pool exists now: the same value is accepted, another one names the order */
  headtrackr.camshift.pairSchedule = 'cluster';
  threw = false;
  try { headtrackr.camshift.pairSchedule = 'workgroup'; } catch (e) { threw = !(e instanceof RangeError) && /before the first camshift\.Tracker/.test(e.message); }
  check(threw && headtrackr.camshift.pairSchedule === 'cluster', 'camshift.pairSchedule after the pool exists must throw an Error naming the order');
  out.setter_refused = threw;
};
